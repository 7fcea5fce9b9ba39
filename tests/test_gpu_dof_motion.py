"""The joint-angle motion sampler on the MI355X (rtg.h rtg_dof_motion_sample_f32, ops.dof_motion_sample,
rtg.motion.DofMotionLibrary): every output equals the composition of oracle primitives (tests/dof_motion_ref.py) bit
for bit, NaN as NaN, the sign of zero included -- on three models (one joint, Hu v5, a random 64-joint tree: both tile
shapes), ragged launches, every flag and output combination, hostile angles, root rotations and times, single bad
rows, invalid queries, and through the drop-in class.  No query is skipped or masked."""
import ctypes

import numpy as np
import pytest
import torch

import dof_motion_ref as ref
import motion_sample_ref as msr
from dof_motion_ref import KEYS, bits

pytestmark = pytest.mark.gpu

SKELETONS = ("one", "hu_v5", "rand64")
_MODELS, _HANDLES, _BASE = {}, {}, {}


def model(name):
    """The reference-side model dict: the one-joint chain, Hu v5 (31) and a random 64-joint tree, random axes and
    limits per DOF."""
    if name not in _MODELS:
        from rtg import assets
        if name == "one":
            p, lt = np.array([-1], np.int32), np.zeros((1, 3), np.float32)
        elif name == "rand64":
            p, lt, _ = msr.random_tree(64)
        else:
            p, lt = assets.parents(name).astype(np.int32), assets.local_translation(name).astype(np.float32)
        _MODELS[name] = ref.make_model(p, lt)
    return _MODELS[name]


def handle(name, limits=True):
    """The device-side DofModel (with or without limits)."""
    if (name, limits) not in _HANDLES:
        from rtg.runtime import DofModel, Topology
        m = model(name)
        topo = Topology(m["parents"], m["local_t"])
        _HANDLES[name, limits] = DofModel(topo, m["axis"], m["lower"] if limits else None, m["upper"] if limits else None)
    return _HANDLES[name, limits]


def frames_per_wave(J):
    return 16 if J <= 36 else 8


class DevLib:
    """A helper-format library on the device."""

    def __init__(self, lib):
        from rtg.runtime import MotionLib
        self.host = lib
        self.dof, self.root_rot, self.root_t = (torch.from_numpy(lib[k]).cuda() for k in ("dof", "root_rot", "root_t"))
        self.handle = MotionLib(lib["start"], lib["len"], lib["fps"], len(lib["root_rot"]))


FULL = dict(normalize=True, clip_angles=True, velocity=True, want_global=True)


def run(name, dl, clip, time, normalize=False, clip_angles=False, velocity=True, want_global=True, key_links=None):
    from rtg import ops
    r = ops.dof_motion_sample(handle(name), dl.handle, dl.dof, dl.root_rot, dl.root_t,
                              torch.from_numpy(np.asarray(clip, np.int32)), torch.from_numpy(np.asarray(time, np.float32)),
                              normalize=normalize, clip=clip_angles, want_velocity=velocity, want_global=want_global,
                              key_links=key_links)
    torch.cuda.synchronize()
    return {k: None if x is None else x.cpu().numpy() for k, x in zip(KEYS, r)}


def want(name, lib, clip, time, normalize=False, clip_angles=False, velocity=True, want_global=True, key_links=None):
    return ref.sample(lib, clip, time, normalize, velocity, model(name), clip_angles, want_global, key_links)


def same(got, exp, msg=""):
    for k in KEYS:
        assert (got[k] is None) == (exp[k] is None), (k, msg)
        if got[k] is not None:
            assert got[k].shape == exp[k].shape, (k, msg, got[k].shape, exp[k].shape)
            np.testing.assert_array_equal(bits(got[k]), bits(exp[k]), err_msg=f"{k} {msg}")


def queries(lib, n, seed=0):
    """Every time family on every clip, then random (clip, time) pairs up to n queries."""
    c, t = msr.library_queries(lib)
    rng = np.random.default_rng(seed)
    m = max(0, n - len(c))
    rc = rng.integers(0, len(lib["len"]), m).astype(np.int32)
    dur = (lib["len"][rc] - 1) / lib["fps"][rc]
    rt = (rng.uniform(-0.05, 1.1, m) * dur).astype(np.float32)
    return np.concatenate([c, rc])[:n], np.concatenate([t, rt])[:n]


def keys_of(name):
    J = len(model(name)["parents"])
    return [J - 1, 0, J // 2, 0, min(5, J - 1), J - 1]       # link 0, the last link, duplicates


def base(name, n=4097):
    """Per model, computed once and left unchanged: the smooth library, its device copy, n queries and the reference
    of the fullest combination."""
    if name not in _BASE:
        lib = ref.make_library(len(model(name)["parents"]) - 1, "smooth")
        c, t = queries(lib, n)
        _BASE[name] = (lib, DevLib(lib), c, t, want(name, lib, c, t, key_links=keys_of(name), **FULL))
    return _BASE[name]


def head(w, lo, hi=None):
    s = slice(lo, hi) if hi is not None else slice(0, lo)
    return {k: None if w[k] is None else w[k][s] for k in KEYS}


# ------------------------------------------------------------------------------------------------ the launch
@pytest.mark.parametrize("name", SKELETONS)
def test_tile_edges_every_time_family_and_two_launches(gpu, name):
    lib, dl, c, t, w = base(name)
    F = frames_per_wave(len(model(name)["parents"]))
    assert len(c) == 4097 and np.isnan(t).any() and np.signbit(t[t == 0]).any() and (t < 0).any() and (t > 1e38).any()
    assert (w["b"] == 1).any() and (w["row0"] == w["row1"]).any() and (w["row1"] == w["row0"] + 1).any()
    K = keys_of(name)
    for N in (1, F - 1, F, F + 1, 4097):
        got = run(name, dl, c[:N], t[:N], key_links=K, **FULL)
        same(got, head(w, N), f"N={N}")
    h = 2048 + 5                                               # two launches over the two (ragged) halves
    same(run(name, dl, c[:h], t[:h], key_links=K, **FULL), head(w, h), "first half")
    same(run(name, dl, c[h:], t[h:], key_links=K, **FULL), head(w, h, 4097), "second half")
    empty = run(name, dl, c[:0], t[:0], key_links=K, **FULL)   # N = 0: a no-op
    J = len(model(name)["parents"])
    assert empty["dof"].shape == (0, J - 1) and empty["g_pos"].shape == (0, J, 3) and empty["key_pos"].shape == (0, 6, 3)


@pytest.mark.parametrize("name", SKELETONS)
def test_a_query_does_not_depend_on_its_place(gpu, name):
    lib, dl, c, t, w = base(name)
    N = 1000
    perm = np.random.default_rng(5).permutation(N)
    got = run(name, dl, c[:N][perm], t[:N][perm], key_links=keys_of(name), **FULL)
    same(got, {k: w[k][:N][perm] for k in KEYS}, "permuted")


OUTPUT_SETS = {"local": dict(velocity=False, want_global=False, keys=False),
               "velocities": dict(velocity=True, want_global=False, keys=False),
               "global": dict(velocity=False, want_global=True, keys=False),
               "keys_only": dict(velocity=False, want_global=False, keys=True),
               "everything": dict(velocity=True, want_global=True, keys=True)}
SENTINEL = 0x7FA5A5A5   # a NaN no kernel here writes


@pytest.mark.parametrize("name", SKELETONS)
@pytest.mark.parametrize("normalize", (False, True))
@pytest.mark.parametrize("clip_angles", (False, True))
@pytest.mark.parametrize("outputs", list(OUTPUT_SETS))
def test_every_flag_and_output_combination_and_nothing_else_written(gpu, name, normalize, clip_angles, outputs):
    """Through the C ABI with every output carved out of one sentinel-filled arena, 64 floats of guard around each: the
    outputs asked for equal the reference, and every other float of the arena -- the guards and the room of the outputs
    not asked for -- still holds the sentinel."""
    from rtg import _lib
    lib, dl, c, t, _ = base(name)
    o = OUTPUT_SETS[outputs]
    J = len(model(name)["parents"])
    nd = J - 1
    N = 3 * frames_per_wave(J) + 5
    c, t = np.concatenate([c[:N], c[-N:]]), np.concatenate([t[:N], t[-N:]])
    N = len(c)
    K = keys_of(name) if o["keys"] else []
    exp = want(name, lib, c, t, normalize, clip_angles, o["velocity"], o["want_global"], K)
    widths = dict(dof=nd, dof_vel=nd, root_rot=4, root_t=3, root_vel=6, g_rot=J * 4, g_pos=J * 3, key_pos=3 * 6)
    asked = dict(dof=True, dof_vel=o["velocity"], root_rot=True, root_t=True, root_vel=o["velocity"],
                 g_rot=o["want_global"], g_pos=o["want_global"], key_pos=o["keys"])
    G, off, at = 64, 64, {}
    for k in KEYS:
        at[k] = off
        off += (N * widths[k] + 3) // 4 * 4 + G
    arena = torch.full((off,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    cd, td = torch.from_numpy(c).cuda(), torch.from_numpy(t).cuda()
    ka = np.asarray(K, np.int32)

    def p(k):   # a one-joint model has no angle rows: no address to give
        return ctypes.c_void_p(arena.data_ptr() + 4 * at[k]) if asked[k] and N * widths[k] else None

    L = _lib.lib()
    rc = L.rtg_dof_motion_sample_f32(handle(name).handle, dl.handle.handle, dl.dof.data_ptr() if nd else None,
                                     dl.root_rot.data_ptr(), dl.root_t.data_ptr(), cd.data_ptr(), td.data_ptr(), N,
                                     (1 if normalize else 0) | (2 if clip_angles else 0),
                                     ka.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if len(K) else None, len(K),
                                     p("dof"), p("dof_vel"), p("root_rot"), p("root_t"), p("root_vel"), p("g_rot"),
                                     p("g_pos"), p("key_pos"), None)
    assert rc == 0, L.rtg_last_error().decode()
    torch.cuda.synchronize()
    raw = arena.cpu().numpy()
    untouched = np.ones(off, bool)
    for k in KEYS:
        if asked[k]:
            n = N * widths[k]
            untouched[at[k]:at[k] + n] = False
            assert exp[k] is not None
            np.testing.assert_array_equal(bits(raw[at[k]:at[k] + n]), bits(exp[k].reshape(-1)), err_msg=k)
        else:
            assert exp[k] is None
    assert (raw.view(np.uint32)[untouched] == SENTINEL).all()


@pytest.mark.parametrize("name", SKELETONS)
@pytest.mark.parametrize("clip_angles", (False, True))
def test_global_outputs_equal_dof_fk_of_the_local_outputs_and_key_links_are_its_rows(gpu, name, clip_angles):
    """Device against device: g_rot / g_pos are rtg_dof_fk_f32 on this launch's own dof_out, root_rot_out, root_t_out with
    the same clip flag; key_pos is g_pos[:, links] -- duplicates, link 0, K = 32 -- with and without the global rows."""
    from rtg import ops
    lib, dl, c, t, _ = base(name)
    N, J = 777, len(model(name)["parents"])
    links = [(7 * k) % J for k in range(30)] + [0, 0]
    assert len(links) == 32
    cd, td = torch.from_numpy(c[:N]), torch.from_numpy(t[:N])
    r = ops.dof_motion_sample(handle(name), dl.handle, dl.dof, dl.root_rot, dl.root_t, cd, td, normalize=True,
                              clip=clip_angles, key_links=links)
    fr, fp = ops.dof_forward_kinematics(handle(name), r.dof, r.root_rot, r.root_t, clip=clip_angles)
    np.testing.assert_array_equal(bits(r.g_rot.cpu().numpy()), bits(fr.cpu().numpy()))
    np.testing.assert_array_equal(bits(r.g_pos.cpu().numpy()), bits(fp.cpu().numpy()))
    np.testing.assert_array_equal(bits(r.key_pos.cpu().numpy()), bits(r.g_pos[:, links].cpu().numpy()))
    only = ops.dof_motion_sample(handle(name), dl.handle, dl.dof, dl.root_rot, dl.root_t, cd, td, normalize=True,
                                 clip=clip_angles, want_velocity=False, want_global=False, key_links=links)
    assert only.g_rot is None and only.g_pos is None and only.dof_vel is None and only.root_vel is None
    np.testing.assert_array_equal(bits(only.key_pos.cpu().numpy()), bits(r.key_pos.cpu().numpy()))
    one = ops.dof_motion_sample(handle(name), dl.handle, dl.dof, dl.root_rot, dl.root_t, cd, td, normalize=True,
                                clip=clip_angles, want_global=False, key_links=[J - 1])
    np.testing.assert_array_equal(bits(one.key_pos.cpu().numpy()), bits(r.g_pos[:, [J - 1]].cpu().numpy()))


# ------------------------------------------------------------------------------------------------ hostile rows
HOSTILE_ANGLES = np.array([0.0, -0.0, 1e-40, -1e-40, np.pi, -np.pi, 1e4, -1e4, 1e18, np.inf, -np.inf, np.nan, 0.3],
                          np.float32)


@pytest.mark.parametrize("name", ("hu_v5", "rand64"))
def test_hostile_angles(gpu, name):
    """Every ordered pair of hostile angles as consecutive frames of every DOF (the sequence a, b over all (a, b),
    rotated from DOF to DOF), queried at and between every consecutive pair, clipped and not."""
    nd = len(model(name)["parents"]) - 1
    n = len(HOSTILE_ANGLES)
    seq = np.array([x for a in range(n) for b in range(n) for x in (a, b)])
    L = len(seq)
    idx = seq[(np.arange(L)[:, None] + 3 * np.arange(nd)[None, :]) % L]
    lib = ref.make_library(nd, "smooth", lengths=(L, 3), fps=(30.0, 1.0), seed=2)
    lib["dof"][:L] = HOSTILE_ANGLES[idx]
    assert len({(int(a), int(b)) for a, b in zip(idx[:-1, 0], idx[1:, 0])}) == n * n
    c, t = msr.library_queries(lib)
    dl = DevLib(lib)
    for clip_angles in (False, True):
        same(run(name, dl, c, t, True, clip_angles, True, True, keys_of(name)),
             want(name, lib, c, t, True, clip_angles, True, True, keys_of(name)), f"clip={clip_angles}")


def test_subnormal_velocity_quotients(gpu):
    """Differences of tiny angles and root translations over frame times of 1, 4, 1/3 s and more: quotients that are
    subnormal, exact and inexact, next to a subnormal dt (3e38 fps) and a huge one."""
    name = "hu_v5"
    fps = (1.0, 0.25, 3.0, 3e38, 1e-30)
    lib = ref.make_library(30, "smooth", lengths=(9,) * 5, fps=fps, seed=3)
    rng = np.random.default_rng(8)
    tiny = (rng.integers(-2000, 2000, lib["dof"].shape) * np.float64(2.0 ** -149)).astype(np.float32)
    lib["dof"] = tiny
    lib["root_t"] = (rng.integers(-99, 99, lib["root_t"].shape) * np.float64(2.0 ** -147)).astype(np.float32)
    c = np.repeat(np.arange(5, dtype=np.int32), 8)
    with np.errstate(all="ignore"):
        t = ((np.tile(np.arange(8), 5) + 0.5) / np.asarray(fps, np.float64)[c]).astype(np.float32)
    exp = want(name, lib, c, t, True, False, True, False)
    v = exp["dof_vel"][np.isfinite(exp["dof_vel"])]
    assert ((v != 0) & (np.abs(v) < 2.0 ** -126)).sum() > 100 and (np.abs(v) >= 2.0 ** -126).any()
    same(run(name, DevLib(lib), c, t, True, False, True, False), exp)


@pytest.mark.parametrize("family", msr.ROT_FAMILIES)
def test_hostile_root_rotations(gpu, family):
    """Every rotation family of kinematics_frames on the root (non-unit, near-unit, tiny, huge, zero, NaN, antipodal
    pairs), queried at and between every consecutive frame pair; the angular velocity of every pair with it."""
    name = "hu_v5"
    lib = ref.make_library(30, family, seed=11)
    c, t = msr.library_queries(lib)
    dl = DevLib(lib)
    for normalize in (True, False):
        same(run(name, dl, c, t, normalize, False, True, True, [0, 30]),
             want(name, lib, c, t, normalize, False, True, True, [0, 30]), family)


def test_slerp_threshold_pairs_on_the_root(gpu):
    name = "hu_v5"
    tl, names = msr.threshold_library(1)
    n = len(names)
    lib = ref.make_library(30, "smooth", lengths=(2,) * n, fps=(1.0,) * n, seed=5)
    lib["root_rot"] = np.ascontiguousarray(tl["rot"][:, 0])
    bs = np.array([0.0, 0.25, 0.5, 0.75, np.nextafter(np.float32(1), np.float32(0))], np.float32)
    c = np.repeat(np.arange(n, dtype=np.int32), len(bs))
    t = np.tile(bs, n)                                        # fps 1: the time is the blend factor
    dl = DevLib(lib)
    for normalize in (False, True):
        same(run(name, dl, c, t, normalize, False, True, True), want(name, lib, c, t, normalize, False, True, True))


@pytest.mark.parametrize("name", ("hu_v5", "rand64"))
@pytest.mark.parametrize("kind", ("nan_angle", "inf_angle", "nan_root", "antipodal_root", "zero_root"))
def test_one_bad_row_among_ordinary_ones(gpu, name, kind):
    """One bad value at a moving query -- both sides of every tile boundary, the first and the last lane of a wave
    instruction -- among smooth rows: query n blends frames n and n + 1, so only queries n - 1 and n may change."""
    J = len(model(name)["parents"])
    nd, F = J - 1, frames_per_wave(J)
    N = 3 * F
    lib0 = ref.make_library(nd, "smooth", lengths=(N + 1,), fps=(30.0,), seed=21)
    c = np.zeros(N, np.int32)
    t = ((np.arange(N) + 0.5) / 30.0).astype(np.float32)
    assert (msr.index_rule(c, t, lib0["len"], lib0["fps"])[1] == np.arange(N)).all()
    dl0 = DevLib(lib0)
    K = keys_of(name)
    clean = run(name, dl0, c, t, key_links=K, **FULL)
    same(clean, want(name, lib0, c, t, key_links=K, **FULL), "clean")
    lane63 = [(r // nd, r % nd) for r in range(63, N * nd, 64)]
    spots = {(n, d) for n in (1, F - 1, F, 2 * F - 1, 2 * F, 3 * F - 1) for d in (0, nd // 2, nd - 1)}
    spots |= {lane63[0], lane63[-1]}
    for n, d in sorted(s for s in spots if s[0] >= 1):
        lib = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in lib0.items()}
        if kind == "nan_angle":
            lib["dof"][n, d] = np.nan
        elif kind == "inf_angle":
            lib["dof"][n, d] = np.inf
        elif kind == "nan_root":
            lib["root_rot"][n, d % 4] = np.nan
        elif kind == "antipodal_root":
            lib["root_rot"][n] = -lib["root_rot"][n - 1]
        else:
            lib["root_rot"][n] = 0.0
        got = run(name, DevLib(lib), c, t, key_links=K, **FULL)
        same(got, want(name, lib, c, t, key_links=K, **FULL), f"{kind} {n},{d}")
        keep = np.setdiff1d(np.arange(N), [n - 1, n])          # row n is frame 1 of query n - 1 and frame 0 of query n
        for k in KEYS:
            np.testing.assert_array_equal(bits(got[k][keep]), bits(clean[k][keep]), err_msg=f"{k} {n},{d}")


def test_clip_boundaries_are_adjacent_rows_and_never_crossed(gpu):
    """The last frame of clip c and the first of clip c + 1 are adjacent rows: a query at or past the end of clip c
    returns clip c's last frame exactly with zero velocities, whatever follows it -- the neighbours' rows poisoned."""
    name = "hu_v5"
    lib, dl, _, _, _ = base(name)
    C = len(lib["len"])
    c = np.repeat(np.arange(C, dtype=np.int32), 4)
    end = (lib["len"] - 1) / lib["fps"].astype(np.float64)
    t = np.stack([np.nextafter(end.astype(np.float32), np.float32(-1)), end, end * 1.5 + 0.01, np.full(C, np.inf)],
                 1).reshape(-1).astype(np.float32)
    got = run(name, dl, c, t, True, False, True, True, [0, 30])
    same(got, want(name, lib, c, t, True, False, True, True, [0, 30]))
    for k in range(C):                                        # clip k alone intact, every other row NaN
        lo, hi = int(lib["start"][k]), int(lib["start"][k] + lib["len"][k])
        p = {x: (np.full_like(lib[x], np.nan) if x in ("dof", "root_rot", "root_t") else lib[x]) for x in lib}
        for x in ("dof", "root_rot", "root_t"):
            p[x][lo:hi] = lib[x][lo:hi]
        m = c == k
        alone = run(name, DevLib(p), c[m], t[m], True, False, True, True, [0, 30])
        same(alone, {x: got[x][m] for x in KEYS}, f"clip {k}")
        assert not np.isnan(alone["dof"]).any() and not np.isnan(alone["root_vel"]).any()
        _, i0, i1, _ = msr.index_rule(c[m], t[m], lib["len"], lib["fps"])
        past = i0 == i1
        if past.any():
            np.testing.assert_array_equal(bits(alone["dof"][past]), bits(np.repeat(lib["dof"][hi - 1:hi], past.sum(), 0)))
            assert (bits(alone["dof_vel"][past]) == 0).all() and (bits(alone["root_vel"][past]) == 0).all()


@pytest.mark.parametrize("name", SKELETONS)
def test_invalid_queries_are_quiet_nan_and_leave_the_rest_alone(gpu, name):
    lib, dl, c, t, _ = base(name)
    J = len(model(name)["parents"])
    F = frames_per_wave(J)
    N = 3 * F + 5
    c, t = c[100:100 + N].copy(), t[100:100 + N].copy()
    K = keys_of(name)
    clean = run(name, dl, c, t, key_links=K, **FULL)
    bad = {0: -1, F - 1: len(lib["len"]), F + F // 2: -1, 2 * F: len(lib["len"]), N - 1: 2**31 - 1, F: -2**31}
    cb = c.copy()
    for n, v in bad.items():
        cb[n] = v
    got = run(name, dl, cb, t, key_links=K, **FULL)
    same(got, want(name, lib, cb, t, key_links=K, **FULL))
    rows = sorted(bad)
    keep = np.setdiff1d(np.arange(N), rows)
    for k in KEYS:
        raw = got[k][rows].view(np.uint32)
        assert (raw == 0x7FC00000).all(), k          # the raw bits: the quiet NaN itself, not merely a NaN
        np.testing.assert_array_equal(bits(got[k][keep]), bits(clean[k][keep]), err_msg=k)
    only = run(name, dl, cb, t, True, True, False, False, K)   # the key links without the global rows
    np.testing.assert_array_equal(bits(only["key_pos"]), bits(got["key_pos"]))
    assert (only["key_pos"][rows].view(np.uint32) == 0x7FC00000).all()


# ------------------------------------------------------------------------------------------------ the drop-in level
def test_dof_motion_library_end_to_end(gpu):
    """fit_pose-shaped tuples ((L, J-1, 1) angles, (L, 3), (L, 1, 4), fps) and plain ones through
    HuForwardModel.motion_library: the packing, the properties, sample() against the ops call and the reference, key
    links by name."""
    from poselib.poselib.skeleton.skeleton3d import SkeletonTree
    from robot_kinematics_model.hu_forward_model import HuForwardModel
    from rtg import ops
    from rtg.motion import DofMotionLibrary, DofMotionSample
    m = model("hu_v5")
    names = [f"link{i}" for i in range(31)]
    tr = SkeletonTree(names, torch.from_numpy(m["parents"].astype(np.int64)), torch.from_numpy(m["local_t"]))
    hu = HuForwardModel(tr, dof_axis=[int(a) for a in m["axis"]], dof_lower=m["lower"], dof_upper=m["upper"])
    lib = ref.make_library(30, "smooth", lengths=(40, 17), fps=(30.0, 120.0), seed=9)
    a, b = slice(0, 40), slice(40, 57)
    T = torch.from_numpy
    clips = [(T(lib["dof"][a])[..., None], T(lib["root_t"][a]), T(lib["root_rot"][a])[:, None], 30),
             (T(lib["dof"][b]).cuda(), lib["root_t"][b], T(lib["root_rot"][b]), 120.0)]
    ml = hu.motion_library(clips)
    assert isinstance(ml, DofMotionLibrary)
    assert ml.num_clips == 2 and list(ml.lengths) == [40, 17] and list(ml.fps) == [30.0, 120.0]
    np.testing.assert_allclose(ml.durations, [39 / 30, 16 / 120])
    for got, exp in ((ml.dof, lib["dof"]), (ml.root_t, lib["root_t"]), (ml.root_rot, lib["root_rot"])):
        assert got.is_cuda and got.dtype == torch.float32
        np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(exp))
    c, t = queries(lib, 300, seed=3)
    c[7] = 2                                                   # an invalid query among them
    links = ["link30", "link0", 12, "link5"]
    idx = [30, 0, 12, 5]
    for kw in (dict(), dict(clip_angles=True, normalize=False), dict(want_global=False, want_velocity=False),
               dict(want_global=False, key_links=None)):
        kw = dict(dict(key_links=links), **kw)
        s = ml.sample(c, t, **kw)
        assert isinstance(s, DofMotionSample)
        k = None if kw["key_links"] is None else idx
        r = ops.dof_motion_sample(hu._model, ml._lib, ml.dof, ml.root_rot, ml.root_t, c, t,
                                  normalize=kw.get("normalize", True), clip=kw.get("clip_angles", False),
                                  want_velocity=kw.get("want_velocity", True), want_global=kw.get("want_global", True),
                                  key_links=k)
        w = ref.sample(lib, c, t, kw.get("normalize", True), kw.get("want_velocity", True), m,
                       kw.get("clip_angles", False), kw.get("want_global", True), k)
        rv, wv = r.root_vel, w["root_vel"]
        for got, dev, exp in ((s.dof_pos, r.dof, w["dof"]), (s.dof_vel, r.dof_vel, w["dof_vel"]),
                              (s.root_translation, r.root_t, w["root_t"]), (s.root_rotation, r.root_rot, w["root_rot"]),
                              (s.root_velocity, None if rv is None else rv[:, :3], None if wv is None else wv[:, :3]),
                              (s.root_angular_velocity, None if rv is None else rv[:, 3:], None if wv is None else wv[:, 3:]),
                              (s.global_rotation, r.g_rot, w["g_rot"]), (s.global_translation, r.g_pos, w["g_pos"]),
                              (s.key_translation, r.key_pos, w["key_pos"])):
            assert (got is None) == (exp is None) == (dev is None)
            if got is not None:
                assert got.is_cuda
                np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(dev.cpu().numpy()))
                np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(exp))
    with pytest.raises(ValueError, match="no node named"):
        ml.sample(c, t, key_links=["nose"])
    one = DofMotionLibrary(hu, clips[0])                        # one clip, not a list
    assert one.num_clips == 1 and list(one.lengths) == [40]
    no_limits = DofMotionLibrary(handle("hu_v5", limits=False), clips)
    with pytest.raises(ValueError, match="limits"):
        no_limits.sample(c, t, clip_angles=True)


# ------------------------------------------------------------------------------------------------ error paths
def test_error_paths_on_the_device(gpu):
    from rtg import _lib, ops
    from rtg.runtime import DofModel, MotionLib, Topology
    name = "hu_v5"
    lib, dl, c, t, _ = base(name)
    h = handle(name)
    args = (dl.dof, dl.root_rot, dl.root_t)
    # the wrapper: shapes against F_total, dtypes, the device, the limits, the key links
    for bad in ((dl.dof[:-1], dl.root_rot, dl.root_t), (dl.dof, dl.root_rot[:-1], dl.root_t),
                (dl.dof, dl.root_rot, dl.root_t[:-1]), (dl.dof[:, :-1], dl.root_rot, dl.root_t)):
        with pytest.raises(ValueError):
            ops.dof_motion_sample(h, dl.handle, *bad, c[:4], t[:4])
    with pytest.raises(ValueError):
        ops.dof_motion_sample(h, dl.handle, *args, c[:4], t[:5])
    with pytest.raises(ValueError, match="integers"):
        ops.dof_motion_sample(h, dl.handle, *args, c[:4].astype(np.float32), t[:4])
    with pytest.raises(ValueError, match="limits"):
        ops.dof_motion_sample(handle(name, limits=False), dl.handle, *args, c[:4], t[:4], clip=True)
    with pytest.raises(ValueError, match="key_links"):
        ops.dof_motion_sample(h, dl.handle, *args, c[:4], t[:4], key_links=[31])
    with pytest.raises(ValueError, match="at most 32"):
        ops.dof_motion_sample(h, dl.handle, *args, c[:4], t[:4], key_links=[0] * 33)
    elsewhere = MotionLib(lib["start"], lib["len"], lib["fps"], len(lib["root_rot"]))
    elsewhere.device = torch.device("cuda", torch.cuda.current_device() + 1)
    with pytest.raises(ValueError, match="lives on"):
        ops.dof_motion_sample(h, elsewhere, *args, c[:4], t[:4])
    d64 = ops.dof_motion_sample(h, dl.handle, dl.dof.double().cpu(), dl.root_rot.cpu(), dl.root_t.double(), c[:40], t[:40])
    np.testing.assert_array_equal(bits(d64.dof.cpu().numpy()), bits(want(name, lib, c[:40], t[:40])["dof"]))

    # the C ABI's checks behind live handles, all before any launch
    L = _lib.lib()
    N, J = 8, 31
    cd, td = torch.from_numpy(c[:N]).cuda(), torch.from_numpy(t[:N]).cuda()
    out = torch.empty(4096, device="cuda")
    o_dof, o_rr, o_rt, o_g = out.data_ptr(), out.data_ptr() + 4096, out.data_ptr() + 4096 + 256, out.data_ptr() + 8192

    def call(model=None, flags=0, keys=(), dof=dl.dof.data_ptr(), do=o_dof, rro=o_rr, rto=o_rt, rv=None, dv=None,
             gr=None, gp=None, kp=None, n=N):
        ka = np.asarray(keys, np.int32)
        rc = L.rtg_dof_motion_sample_f32((model or h).handle, dl.handle.handle, dof, dl.root_rot.data_ptr(),
                                         dl.root_t.data_ptr(), cd.data_ptr(), td.data_ptr(), n, flags,
                                         ka.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if len(ka) else None, len(ka),
                                         do, dv, rro, rto, rv, gr, gp, kp, None)
        return rc, L.rtg_last_error().decode()

    fn = "rtg_dof_motion_sample_f32: "
    rc, msg = call(model=handle(name, limits=False), flags=_lib.DOF_MOTION_CLIP)
    assert rc == 1 and msg.startswith(fn) and "no DOF limits" in msg, msg
    rc, msg = call(keys=[0, 31], kp=o_g)
    assert rc == 1 and msg.startswith(fn) and "key_links[1]=31 is outside 0..30" in msg, msg
    p65 = np.arange(-1, 64, dtype=np.int32)
    m65 = DofModel(Topology(p65, np.zeros((65, 3), np.float32)), np.zeros(64, np.int32))
    rc, msg = call(model=m65)
    assert rc == 4 and msg.startswith(fn) and "65" in msg, msg                     # RTG_ERR_UNSUPPORTED
    rc, msg = call(n=0, model=m65)
    assert rc == 4, msg                                                            # the checks come before the no-op
    rc, msg = call(dof=None)
    assert rc == 1 and "NULL buffer" in msg, msg
    rc, msg = call(do=None)
    assert rc == 1 and "NULL buffer" in msg, msg
    rc, msg = call(rv=o_g)
    assert rc == 1 and "dof_vel_out" in msg, msg
    for kw in (dict(do=dl.dof.data_ptr() + 4 * 30), dict(rto=dl.root_t.data_ptr() + 12), dict(rro=dl.root_rot.data_ptr() + 16),
               dict(rto=o_dof + 4), dict(keys=[1], kp=o_rr), dict(gr=o_g, gp=o_g + 16), dict(dv=o_g, rv=o_g + 8)):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(fn) and "overlap" in msg, (kw, msg)
    rc, msg = call(rro=o_rr + 4)
    assert rc == 1 and "aligned" in msg, msg
    rc, msg = call(n=0)
    assert rc == 0, msg
    rc, msg = call()
    assert rc == 0, msg
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(out[:N * 30].cpu().numpy().reshape(N, 30)), bits(want(name, lib, c[:N], t[:N])["dof"]))

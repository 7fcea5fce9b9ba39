"""Link velocities from joint velocities on the MI355X (rtg.h rtg_dof_fk_vel_f32, rtg_dof_motion_sample_vel_f32;
ops.dof_link_velocity, ops.dof_motion_sample's new keywords, DofMotionLibrary.sample(link_velocities=True),
HuForwardModel.link_velocities): every output equals the restatement of the rule (tests/fk_velocity_ref.py) bit for
bit, NaN as NaN, the sign of zero included -- on five models (one joint, two joints, Hu v5, a random 37-joint tree:
the first with 8 frames per wave, a random 64-joint tree), ragged launches on both sides of every tile size, clip on
and off with angles at a limit and one ulp past it, hostile rates and twists, single bad elements, sentinel-filled
arenas, every output set of the sampler, invalid queries, times past a clip's end, and the rejections that need live
handles."""
import ctypes

import numpy as np
import pytest
import torch

import dof_motion_ref as dmr
import fk_velocity_ref as ref
import motion_sample_ref as msr
from fk_velocity_ref import bits

pytestmark = pytest.mark.gpu

MODELS = ("one", "two", "hu_v5", "rand37", "rand64")
SENTINEL = 0x7FA5A5A5   # a NaN no kernel here writes
_MODELS, _HANDLES, _FRAMES, _LIBS = {}, {}, {}, {}


def model(name):
    if name not in _MODELS:
        from rtg import assets
        if name == "one":
            p, lt = np.array([-1], np.int32), np.zeros((1, 3), np.float32)
        elif name == "two":
            p, lt = np.array([-1, 0], np.int32), np.array([[0, 0, 0], [0.3, -0.2, 0.5]], np.float32)
        elif name.startswith("rand"):
            p, lt, _ = msr.random_tree(int(name[4:]))
        else:
            p, lt = assets.parents(name).astype(np.int32), assets.local_translation(name).astype(np.float32)
        _MODELS[name] = dmr.make_model(p, lt)
    return _MODELS[name]


def handle(name, limits=True):
    if (name, limits) not in _HANDLES:
        from rtg.runtime import DofModel, Topology
        m = model(name)
        _HANDLES[name, limits] = DofModel(Topology(m["parents"], m["local_t"]), m["axis"],
                                          m["lower"] if limits else None, m["upper"] if limits else None)
    return _HANDLES[name, limits]


def joints(name):
    return len(model(name)["parents"])


def tile(name):
    return 16 if joints(name) <= 36 else 8


def frames(name):
    """Per model, computed once and left unchanged: 4 F + 3 frames -- angles within +-1.5 rad, some exactly at a limit,
    one ulp outside and one ulp inside it, rates ~ N(0, 3), unit roots, twists ~ N(0, 2) -- and the restatement on the
    oracle's poses, clip off and on."""
    if name not in _FRAMES:
        m = model(name)
        J, F = joints(name), tile(name)
        B, nd = 4 * F + 3, J - 1
        rng = np.random.default_rng(900 + J)
        a = rng.uniform(-1.5, 1.5, (B, nd)).astype(np.float32)
        lo, hi = m["lower"], m["upper"]
        edge = np.stack([lo, hi, np.nextafter(lo, np.float32(-9)), np.nextafter(hi, np.float32(9)),
                         np.nextafter(lo, np.float32(9)), np.nextafter(hi, np.float32(-9))]).astype(np.float32)
        pick = rng.integers(0, 12, (B, nd))                     # half of the angles on or next to a limit
        a = np.where(pick < 6, edge[np.minimum(pick, 5), np.arange(nd)[None, :]], a).astype(np.float32)
        q = rng.normal(size=(B, 4))
        q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
        x = dict(a=a, ad=rng.normal(0, 3, (B, nd)).astype(np.float32), q=q, t=rng.normal(0, 0.5, (B, 3)).astype(np.float32),
                 tw=rng.normal(0, 2, (B, 6)).astype(np.float32))
        if nd:
            assert ((a == lo) | (a == hi)).any() and ((a < lo) | (a > hi)).any()
        want = {c: ref.link_twists(m, a, x["ad"], q, x["t"], x["tw"], clip=c) for c in (False, True)}
        if nd > 1:
            assert (bits(want[False][2]) != bits(want[True][2])).any()          # the clip select shows
        _FRAMES[name] = (x, want)
    return _FRAMES[name]


def col(v):
    """A one-DOF model's (B, 1) rows in the (B, 1, 1) form: (1, 1) alone would read as one frame-less row."""
    return v[..., None] if v.shape[1] == 1 else v


def launch(name, x, clip=False, want_pose=True, twist=True, n=None, limits=True):
    from rtg import ops
    s = slice(0, n)
    r = ops.dof_link_velocity(handle(name, limits), col(x["a"][s]), x["q"][s], x["t"][s], col(x["ad"][s]),
                              x["tw"][s] if twist else None, clip=clip, want_pose=want_pose)
    torch.cuda.synchronize()
    return tuple(None if o is None else o.cpu().numpy() for o in r)


def same(got, exp, msg=""):
    assert got.shape == exp.shape, (msg, got.shape, exp.shape)
    np.testing.assert_array_equal(bits(got), bits(exp), err_msg=msg)


def check(name, x, clip, exp=None, msg=""):
    """One launch against dof_forward_kinematics, the restatement on the launch's own poses and on the oracle's, and
    the velocity-only launch.  -> g_vel."""
    from rtg import ops
    m = model(name)
    g_rot, g_pos, g_vel = launch(name, x, clip)
    fr, fp = ops.dof_forward_kinematics(handle(name), torch.from_numpy(col(x["a"])), torch.from_numpy(x["q"]),
                                        torch.from_numpy(x["t"]), clip=clip)
    same(g_rot, fr.cpu().numpy(), f"g_rot {msg}")
    same(g_pos, fp.cpu().numpy(), f"g_pos {msg}")
    own = ref.link_twists(m, x["a"], x["ad"], x["q"], x["t"], x["tw"], clip=clip, poses=(g_rot, g_pos))[2]
    same(g_vel, own, f"g_vel on the launch's own poses {msg}")
    if exp is None:
        exp = ref.link_twists(m, x["a"], x["ad"], x["q"], x["t"], x["tw"], clip=clip)
    same(g_rot, exp[0], f"g_rot against the oracle {msg}")
    same(g_vel, exp[2], f"g_vel on the oracle's poses {msg}")
    only = launch(name, x, clip, want_pose=False)
    assert only[0] is None and only[1] is None
    same(only[2], g_vel, f"velocity-only {msg}")
    return g_vel


# ------------------------------------------------------------------------------------------------ the standalone call
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("clip", (False, True))
def test_every_batch_size_around_the_tile(gpu, name, clip):
    x, want = frames(name)
    F = tile(name)
    for B in (1, F - 1, F, F + 1, 4 * F + 3):
        xb = {k: v[:B] for k, v in x.items()}
        g_vel = check(name, xb, clip, tuple(w[:B] for w in want[clip]), f"B={B}")
        same(g_vel[:, 0], xb["tw"], "row 0 is the root twist")
    # no root twist is a zero twist, +0 in row 0
    z = dict(x, tw=np.zeros_like(x["tw"]))
    none = launch(name, x, clip, twist=False)
    for a, b in zip(none, launch(name, z, clip)):
        same(a, b, "root_vel NULL")
    assert (none[2][:, 0].view(np.uint32) == 0).all()
    empty = launch(name, x, clip, n=0)
    assert empty[2].shape == (0, joints(name), 6)


HOSTILE = np.array([0.0, -0.0, 1e-40, -1e-40, 1e18, -1e18, np.inf, -np.inf, np.nan], np.float32)


@pytest.mark.parametrize("name", ("two", "hu_v5", "rand64"))
@pytest.mark.parametrize("clip", (False, True))
def test_hostile_rates_and_twists(gpu, name, clip):
    """Every hostile value in every rate column and every twist component, a third of the entries each, among ordinary
    ones."""
    x, _ = frames(name)
    rng = np.random.default_rng(77)
    ad, tw = x["ad"].copy(), x["tw"].copy()
    B, nd = ad.shape
    for arr in (ad, tw):
        which = (np.arange(arr.shape[0])[:, None] + np.arange(arr.shape[1])[None, :]) % len(HOSTILE)
        hit = rng.integers(0, 3, arr.shape) == 0
        hit[:len(HOSTILE)] = True                               # the first frames: every value in every column
        arr[hit] = HOSTILE[which][hit]
    for v in HOSTILE[:8]:
        assert (bits(ad) == bits(v)).any() and (bits(tw) == bits(v)).any()
    assert np.isnan(ad).any() and np.isnan(tw).any()
    g_vel = check(name, dict(x, ad=ad, tw=tw), clip)
    assert np.isfinite(g_vel).any() and np.isnan(g_vel).any() and np.isinf(g_vel).any()


@pytest.mark.parametrize("name", ("hu_v5", "rand64"))
def test_one_bad_element_on_both_sides_of_every_tile_boundary(gpu, name):
    """One NaN / inf in a rate, a twist or an angle of one frame: that frame equals the restatement (a bad rate of a
    joint held at its limit is dropped by the clip select) and every other frame equals the clean run."""
    x, want = frames(name)
    F, nd = tile(name), joints(name) - 1
    clean = launch(name, x, True)
    for w, c in zip(want[True], clean):
        same(c, w, "clean")
    B = len(x["a"])
    for n in (0, F - 1, F, 2 * F - 1, 2 * F, 4 * F - 1, 4 * F, B - 1):
        for key, d, val in (("ad", (n * 7) % nd, np.nan), ("tw", n % 6, np.inf), ("a", (n * 5) % nd, np.nan),
                            ("ad", nd - 1, -np.inf)):
            y = {k: v.copy() for k, v in x.items()}
            y[key][n, d] = val
            got = launch(name, y, True)
            exp = ref.link_twists(model(name), y["a"], y["ad"], y["q"], y["t"], y["tw"], clip=True)
            keep = np.setdiff1d(np.arange(B), [n])
            for g, e, c in zip(got, exp, clean):
                same(g, e, f"{key}[{n},{d}]")
                same(g[keep], c[keep], f"neighbours of {key}[{n},{d}]")
            assert key == "ad" or not np.isfinite(got[2][n]).all()


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("pose", (True, False))
def test_nothing_else_is_written(gpu, name, pose):
    """Through the C ABI with the outputs carved out of one sentinel-filled arena, 64 floats of guard around each."""
    from rtg import _lib
    x, want = frames(name)
    J, B = joints(name), len(x["a"])
    widths = dict(g_rot=4 * J, g_pos=3 * J, g_vel=6 * J)
    G, off, at = 64, 64, {}
    for k in widths:
        at[k] = off
        off += (B * widths[k] + 3) // 4 * 4 + G
    arena = torch.full((off,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    d = {k: torch.from_numpy(v).cuda() for k, v in x.items()}

    def p(k):
        return ctypes.c_void_p(arena.data_ptr() + 4 * at[k])

    L = _lib.lib()
    nd = J - 1
    rc = L.rtg_dof_fk_vel_f32(handle(name).handle, d["a"].data_ptr() if nd else None, d["q"].data_ptr(), d["t"].data_ptr(),
                              d["ad"].data_ptr() if nd else None, d["tw"].data_ptr(), B, 1,
                              p("g_rot") if pose else None, p("g_pos") if pose else None, p("g_vel"), None)
    assert rc == 0, L.rtg_last_error().decode()
    torch.cuda.synchronize()
    raw = arena.cpu().numpy()
    untouched = np.ones(off, bool)
    for k, w in zip(widths, want[True]):
        if pose or k == "g_vel":
            n = B * widths[k]
            untouched[at[k]:at[k] + n] = False
            same(raw[at[k]:at[k] + n], w.reshape(-1), k)
    assert (raw.view(np.uint32)[untouched] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ the sampler
class DevLib:
    def __init__(self, lib):
        from rtg.runtime import MotionLib
        self.host = lib
        self.dof, self.root_rot, self.root_t = (torch.from_numpy(lib[k]).cuda() for k in ("dof", "root_rot", "root_t"))
        self.handle = MotionLib(lib["start"], lib["len"], lib["fps"], len(lib["root_rot"]))


def library(name, n=4097):
    """Per model, once: the smooth library, its device copy and n queries -- every time family on every clip (NaN,
    negative, past the end), then random pairs."""
    if name not in _LIBS:
        lib = dmr.make_library(joints(name) - 1, "smooth")
        c, t = msr.library_queries(lib)
        rng = np.random.default_rng(4)
        m = max(0, n - len(c))
        rc = rng.integers(0, len(lib["len"]), m).astype(np.int32)
        rt = (rng.uniform(-0.05, 1.1, m) * (lib["len"][rc] - 1) / lib["fps"][rc]).astype(np.float32)
        _LIBS[name] = (lib, DevLib(lib), np.concatenate([c, rc])[:n], np.concatenate([t, rt])[:n])
    return _LIBS[name]


def keys_of(name):
    J = joints(name)
    return [J - 1, 0, J // 2, 0, min(5, J - 1), J - 1]


FIELDS = ("dof", "dof_vel", "root_rot", "root_t", "root_vel", "g_rot", "g_pos", "key_pos", "g_vel", "key_vel")


def sample(name, dl, c, t, clip=True, **kw):
    from rtg import ops
    r = ops.dof_motion_sample(handle(name), dl.handle, dl.dof, dl.root_rot, dl.root_t,
                              torch.from_numpy(np.asarray(c, np.int32)), torch.from_numpy(np.asarray(t, np.float32)),
                              normalize=True, clip=clip, **kw)
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in zip(FIELDS, r)}


def restate(name, r, clip=True):
    """The rule on a launch's own dof_out, dof_vel_out, root_vel_out and poses."""
    return ref.link_twists(model(name), r["dof"], r["dof_vel"], r["root_rot"], r["root_t"], r["root_vel"], clip=clip,
                           poses=(r["g_rot"], r["g_pos"]))[2]


@pytest.mark.parametrize("name", MODELS)
def test_sampler_every_launch_size_and_output_set(gpu, name):
    lib, dl, c, t = library(name)
    F, J = tile(name), joints(name)
    K = keys_of(name)
    assert np.isnan(t).any() and (t < 0).any() and (t > 1e38).any()
    full = None
    for N in (1, F - 1, F, F + 1, 4097):
        r = sample(name, dl, c[:N], t[:N], key_links=K, want_link_velocity=True, want_key_velocity=True)
        plain = sample(name, dl, c[:N], t[:N], key_links=K)
        for k in FIELDS[:8]:                                    # the pose outputs are the plain launch's
            same(r[k], plain[k], f"{k} N={N}")
        assert plain["g_vel"] is None and plain["key_vel"] is None
        same(r["g_vel"], restate(name, r), f"g_vel N={N}")
        same(r["key_vel"], r["g_vel"][:, K], f"key_vel N={N}")
        same(r["g_vel"][:, 0], r["root_vel"], "row 0 is root_vel_out")
        full = r
    if J > 2:
        assert (bits(full["g_vel"]) != bits(restate(name, full, clip=False))).any()   # clipped angles among them
    N = 4 * F + 3
    head = {k: v[:N] for k, v in full.items()}
    for clip in (True, False):
        w = sample(name, dl, c[:N], t[:N], clip, key_links=K, want_link_velocity=True, want_key_velocity=True)
        same(w["g_vel"], restate(name, w, clip), f"clip={clip}")
        if clip:
            same(w["g_vel"], head["g_vel"], "a query does not depend on the launch's size")
        # without the global rows; key links only; the key links without key velocities
        a = sample(name, dl, c[:N], t[:N], clip, want_global=False, want_link_velocity=True)
        assert a["g_rot"] is None and a["key_pos"] is None and a["key_vel"] is None
        same(a["g_vel"], w["g_vel"], "without the global rows")
        b = sample(name, dl, c[:N], t[:N], clip, want_global=False, key_links=K, want_key_velocity=True)
        assert b["g_rot"] is None and b["g_vel"] is None
        same(b["key_vel"], w["key_vel"], "key links only")
        same(b["key_pos"], w["key_pos"], "key links only")
        links = [(7 * k) % J for k in range(30)] + [0, 0]      # K = 32 with duplicates and link 0
        d = sample(name, dl, c[:N], t[:N], clip, want_global=False, key_links=links, want_key_velocity=True)
        same(d["key_vel"], w["g_vel"][:, links], "K = 32")
        e = sample(name, dl, c[:N], t[:N], clip, key_links=links, want_link_velocity=True)
        assert e["key_vel"] is None
        same(e["g_vel"], w["g_vel"], "g_vel with key positions only")
        same(e["key_pos"], w["g_pos"][:, links], "K = 32 positions")


@pytest.mark.parametrize("name", ("one", "hu_v5", "rand37"))
def test_sampler_invalid_queries_and_times_past_the_end(gpu, name):
    lib, dl, c, t = library(name)
    F, K = tile(name), keys_of(name)
    N = 3 * F + 5
    c, t = c[100:100 + N].copy(), t[100:100 + N].copy()
    kw = dict(key_links=K, want_link_velocity=True, want_key_velocity=True)
    clean = sample(name, dl, c, t, **kw)
    bad = {0: -1, F - 1: len(lib["len"]), F: -2**31, 2 * F: len(lib["len"]), N - 1: 2**31 - 1}
    cb = c.copy()
    for n, v in bad.items():
        cb[n] = v
    got = sample(name, dl, cb, t, **kw)
    rows = sorted(bad)
    keep = np.setdiff1d(np.arange(N), rows)
    for k in ("g_vel", "key_vel"):
        assert (got[k][rows].view(np.uint32) == 0x7FC00000).all(), k     # the quiet NaN itself
        same(got[k][keep], clean[k][keep], k)
    only = sample(name, dl, cb, t, want_global=False, key_links=K, want_key_velocity=True)
    same(only["key_vel"], got["key_vel"], "key links only")
    # at and past a clip's last frame the velocities are +0, the sign included
    C = len(lib["len"])
    ce = np.repeat(np.arange(C, dtype=np.int32), 3)
    end = (lib["len"] - 1) / lib["fps"].astype(np.float64)
    te = np.stack([end, end * 1.5 + 0.01, np.full(C, np.inf)], 1).reshape(-1).astype(np.float32)
    late = sample(name, dl, ce, te, **kw)
    assert (late["g_vel"].view(np.uint32) == 0).all() and (late["key_vel"].view(np.uint32) == 0).all()
    assert np.isfinite(late["g_pos"]).all()


def _sample_c(fn, name, dl, c, t, flags, keys, outs, extra=()):
    """rtg_dof_motion_sample_f32 or _vel_f32 through ctypes; outs: dict of tensors or None in FIELDS[:8] order."""
    ka = np.asarray(keys, np.int32)
    nd = joints(name) - 1
    a = [handle(name).handle, dl.handle.handle, dl.dof.data_ptr() if nd else None, dl.root_rot.data_ptr(),
         dl.root_t.data_ptr(), c.data_ptr(), t.data_ptr(), len(c), flags,
         ka.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if len(ka) else None, len(ka)]
    a += [None if outs[k] is None or outs[k].numel() == 0 else outs[k].data_ptr() for k in FIELDS[:8]]
    return fn(*a, *extra, None)


@pytest.mark.parametrize("name", ("one", "hu_v5", "rand64"))
def test_both_new_outputs_null_is_the_plain_entry(gpu, name):
    from rtg import _lib
    L = _lib.lib()
    lib, dl, c, t = library(name)
    J, N, K = joints(name), 333, keys_of(name)
    cd, td = torch.from_numpy(c[:N]).cuda(), torch.from_numpy(t[:N]).cuda()
    widths = dict(dof=J - 1, dof_vel=J - 1, root_rot=4, root_t=3, root_vel=6, g_rot=4 * J, g_pos=3 * J, key_pos=18)

    def outs():
        return {k: torch.full((N, w), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
                for k, w in widths.items()}

    a, b = outs(), outs()
    assert _sample_c(L.rtg_dof_motion_sample_f32, name, dl, cd, td, 3, K, a) == 0, L.rtg_last_error().decode()
    assert _sample_c(L.rtg_dof_motion_sample_vel_f32, name, dl, cd, td, 3, K, b, (None, None)) == 0, \
        L.rtg_last_error().decode()
    torch.cuda.synchronize()
    for k in widths:
        np.testing.assert_array_equal(a[k].cpu().numpy().view(np.uint32), b[k].cpu().numpy().view(np.uint32), err_msg=k)
    # ... and its messages under its name
    assert _sample_c(L.rtg_dof_motion_sample_vel_f32, name, dl, cd, td, 8, K, b, (None, None)) == 1
    assert L.rtg_last_error().decode().startswith("rtg_dof_motion_sample_f32: unknown flags")


# ------------------------------------------------------------------------------------------------ error paths
def test_rejections_behind_live_handles(gpu):
    from rtg import _lib, ops
    from rtg.runtime import DofModel, Topology
    L = _lib.lib()
    name = "hu_v5"
    x, _ = frames(name)
    h, J, B = handle(name), 31, 8
    d = {k: torch.from_numpy(v[:B]).cuda() for k, v in x.items()}
    out = torch.empty(16384, device="cuda")
    o_r, o_p, o_v = out.data_ptr(), out.data_ptr() + 16384, out.data_ptr() + 32768

    def call(model=None, dof=d["a"].data_ptr(), dv=d["ad"].data_ptr(), rv=d["tw"].data_ptr(), clip=0, gr=o_r, gp=o_p,
             gv=o_v, n=B):
        rc = L.rtg_dof_fk_vel_f32((model or h).handle, dof, d["q"].data_ptr(), d["t"].data_ptr(), dv, rv, n, clip, gr, gp,
                                  gv, None)
        return rc, L.rtg_last_error().decode()

    fn = "rtg_dof_fk_vel_f32: "
    rc, msg = call(model=handle(name, limits=False), clip=1)
    assert rc == 1 and msg.startswith(fn) and "no DOF limits" in msg, msg
    m65 = DofModel(Topology(np.arange(-1, 64, dtype=np.int32), np.zeros((65, 3), np.float32)), np.zeros(64, np.int32))
    rc, msg = call(model=m65)
    assert rc == 4 and msg.startswith(fn) and "65" in msg, msg                     # RTG_ERR_UNSUPPORTED
    assert call(model=m65, n=0)[0] == 4                                            # the checks come before the no-op
    for kw in (dict(dof=None), dict(dv=None)):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(fn) and "NULL buffer" in msg, (kw, msg)
    for kw in (dict(gv=d["ad"].data_ptr()), dict(gv=d["tw"].data_ptr() + 8), dict(gr=d["q"].data_ptr()),
               dict(gv=o_r + 64), dict(gv=o_p + 4), dict(gp=d["a"].data_ptr())):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(fn) and "overlap" in msg, (kw, msg)
    assert call(gr=o_r + 4)[0] == 1 and "aligned" in L.rtg_last_error().decode()
    assert call(n=0)[0] == 0 and call()[0] == 0 and call(rv=None, gr=None, gp=None)[0] == 0
    # a one-joint model: dof and dof_vel are not dereferenced
    q1, t1 = d["q"], d["t"]
    rc = L.rtg_dof_fk_vel_f32(handle("one").handle, None, q1.data_ptr(), t1.data_ptr(), None, d["tw"].data_ptr(), B, 0,
                              None, None, o_v, None)
    assert rc == 0, L.rtg_last_error().decode()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out[8192:8192 + 6 * B].cpu().numpy().view(np.uint32),
                                  x["tw"][:B].reshape(-1).view(np.uint32))
    # the wrapper
    with pytest.raises(ValueError, match="limits"):
        ops.dof_link_velocity(handle(name, limits=False), x["a"], x["q"], x["t"], x["ad"], clip=True)
    with pytest.raises(ValueError, match="dof's shape"):
        ops.dof_link_velocity(h, x["a"], x["q"], x["t"], x["ad"][:5])

    # the sampler's entry
    lib, dl, c, t = library(name)
    cd, td = torch.from_numpy(c[:B]).cuda(), torch.from_numpy(t[:B]).cuda()
    widths = dict(dof=30, dof_vel=30, root_rot=4, root_t=3, root_vel=6, g_rot=124, g_pos=93, key_pos=3)
    o = {k: torch.empty(B, w, device="cuda") for k, w in widths.items()}
    gv, kv = torch.empty(B, J, 6, device="cuda"), torch.empty(B, 1, 6, device="cuda")
    vel = L.rtg_dof_motion_sample_vel_f32
    sfn = "rtg_dof_motion_sample_vel_f32: "

    def scall(keys=(5,), flags=0, hname=name, limits=True, extra=None, **drop):
        oo = {k: (None if k in drop else v) for k, v in o.items()}
        ka = np.asarray(keys, np.int32)
        a = [handle(hname, limits).handle, dl.handle.handle, dl.dof.data_ptr(), dl.root_rot.data_ptr(), dl.root_t.data_ptr(),
             cd.data_ptr(), td.data_ptr(), B, flags, ka.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if len(ka) else None,
             len(ka)] + [None if oo[k] is None else oo[k].data_ptr() for k in FIELDS[:8]]
        rc = vel(*a, *(extra or (gv.data_ptr(), kv.data_ptr())), None)
        return rc, L.rtg_last_error().decode()

    assert scall()[0] == 0, L.rtg_last_error().decode()
    rc, msg = scall(limits=False, flags=_lib.DOF_MOTION_CLIP)
    assert rc == 1 and msg.startswith(sfn) and "no DOF limits" in msg, msg
    rc, msg = scall(keys=[0, 31])
    assert rc == 1 and msg.startswith(sfn) and "key_links[1]=31 is outside 0..30" in msg, msg
    rc, msg = scall(dof_vel=True)
    assert rc == 1 and msg.startswith(sfn) and "dof_vel_out" in msg, msg
    rc, msg = scall(dof_vel=True, root_vel=True)
    assert rc == 1 and msg.startswith(sfn) and "need dof_vel_out and root_vel_out" in msg, msg
    for extra in ((gv.data_ptr(), gv.data_ptr() + 24), (o["g_pos"].data_ptr(), kv.data_ptr()),
                  (gv.data_ptr(), dl.root_t.data_ptr()), (o["root_vel"].data_ptr(), None)):
        rc, msg = scall(extra=extra)
        assert rc == 1 and msg.startswith(sfn) and "overlap" in msg, (extra, msg)
    assert scall(extra=(gv.data_ptr(), None), key_pos=True, keys=())[0] == 0        # K = 0 with g_vel alone
    assert scall(extra=(None, kv.data_ptr()), key_pos=True, g_rot=True, g_pos=True)[0] == 0   # key_vel alone
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the drop-in level
def test_library_and_model_end_to_end(gpu):
    from poselib.poselib.skeleton.skeleton3d import SkeletonTree
    from robot_kinematics_model.hu_forward_model import HuForwardModel
    from rtg import ops
    m = model("hu_v5")
    names = [f"link{i}" for i in range(31)]
    tr = SkeletonTree(names, torch.from_numpy(m["parents"].astype(np.int64)), torch.from_numpy(m["local_t"]))
    hu = HuForwardModel(tr, dof_axis=[int(a) for a in m["axis"]], dof_lower=m["lower"], dof_upper=m["upper"])
    lib = dmr.make_library(30, "smooth", lengths=(40, 17), fps=(30.0, 120.0), seed=9)
    T = torch.from_numpy
    a, b = slice(0, 40), slice(40, 57)
    ml = hu.motion_library([(T(lib["dof"][a])[..., None], T(lib["root_t"][a]), T(lib["root_rot"][a])[:, None], 30),
                            (T(lib["dof"][b]), lib["root_t"][b], T(lib["root_rot"][b]), 120.0)])
    rng = np.random.default_rng(3)
    c = rng.integers(0, 2, 300).astype(np.int32)
    t = (rng.uniform(-0.05, 1.1, 300) * (lib["len"][c] - 1) / lib["fps"][c]).astype(np.float32)
    c[7] = 2                                                   # an invalid query among them
    links, idx = ["link30", "link0", 12], [30, 0, 12]
    plain = ml.sample(c, t, key_links=links)
    assert plain.global_velocity is None and plain.key_velocity is None
    for clip in (False, True):
        s = ml.sample(c, t, key_links=links, clip_angles=clip, link_velocities=True)
        r = {"dof": s.dof_pos, "dof_vel": s.dof_vel, "root_rot": s.root_rotation, "root_t": s.root_translation,
             "root_vel": torch.cat([s.root_velocity, s.root_angular_velocity], 1), "g_rot": s.global_rotation,
             "g_pos": s.global_translation}
        exp = restate("hu_v5", {k: v.cpu().numpy() for k, v in r.items()}, clip)
        same(s.global_velocity.cpu().numpy(), exp[..., :3], "global_velocity")
        same(s.global_angular_velocity.cpu().numpy(), exp[..., 3:], "global_angular_velocity")
        same(s.key_velocity.cpu().numpy(), exp[:, idx, :3], "key_velocity")
        same(s.key_angular_velocity.cpu().numpy(), exp[:, idx, 3:], "key_angular_velocity")
        same(s.global_translation.cpu().numpy(), ml.sample(c, t, clip_angles=clip).global_translation.cpu().numpy())
        k = ml.sample(c, t, key_links=links, clip_angles=clip, want_global=False, link_velocities=True)
        assert k.global_velocity is None and k.global_rotation is None
        same(k.key_velocity.cpu().numpy(), exp[:, idx, :3], "key links only")
        # the model's own call on the sampled state: the same rows (the invalid query's NaN included)
        v, w = hu.link_velocities(s.dof_pos[..., None], s.root_translation, s.root_rotation[:, None], s.dof_vel[..., None],
                                  s.root_velocity, s.root_angular_velocity, clip_angles=clip)
        assert v.is_cuda and v.shape == (300, 31, 3)
        same(v.cpu().numpy(), exp[..., :3], "HuForwardModel.link_velocities")
        same(w.cpu().numpy(), exp[..., 3:], "HuForwardModel.link_velocities")
    x, want = frames("hu_v5")
    v, w = hu.link_velocities(T(x["a"]), T(x["t"]), T(x["q"]), T(x["ad"]))     # CPU tensors in, CPU tensors out; no twist
    g = ops.dof_link_velocity(hu._model, x["a"], x["q"], x["t"], x["ad"])[2].cpu().numpy()
    assert not v.is_cuda
    same(v.numpy(), g[..., :3])
    same(w.numpy(), g[..., 3:])
    v2, w2 = hu.link_velocities(T(x["a"]), T(x["t"]), T(x["q"]), T(x["ad"]), root_angular_velocity=T(x["tw"][:, 3:]))
    z = dict(x, tw=np.concatenate([np.zeros_like(x["tw"][:, :3]), x["tw"][:, 3:]], 1))
    same(w2.numpy(), launch("hu_v5", z)[2][..., 3:])

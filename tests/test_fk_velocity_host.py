"""The link-velocity rule's host side (no GPU): the float32 restatement (tests/fk_velocity_ref.py) against a float64
tangent of a float64 restatement of the model, the clip rule against differences of the clamped model, the adjoint
identity that ties the rule to what rtg_dof_fk_backward_f32 differentiates, and the argument checks of
rtg_dof_fk_vel_f32 / rtg_dof_motion_sample_vel_f32 and of the new Python keywords that need no device.  The rejections
behind live handles are in tests/test_gpu_link_velocity.py."""
import ctypes
import types

import numpy as np
import pytest

import dof_motion_ref as dmr
import fk_velocity_ref as ref
import motion_sample_ref as msr

# name -> (frames, MEASURED, BOUND): per frame, the largest error of the float32 restatement against the float64 central
# differences over the frame's largest magnitude (linear and angular rows apart, the larger of the two), the maximum
# over the frames.  MEASURED is what test_restatement_against_the_float64_tangent prints for these inputs on the
# restatement as it stands; BOUND = 4 x MEASURED, so that a changed operation order (an error of another size: a
# swapped cross product or a parent's rotation for the joint's own is of order 1) does not pass.
BOUNDS = {"hu_v5": (4096, 5.528e-07, 2.211e-06), "rand64": (1024, 7.409e-07, 2.964e-06),
          "two": (4096, 3.705e-07, 1.482e-06)}


def tree(name):
    if name == "hu_v5":
        from rtg import assets
        return dmr.make_model(assets.parents("hu_v5"), assets.local_translation("hu_v5"))
    if name == "rand64":
        p, lt, _ = msr.random_tree(64)
        return dmr.make_model(p, lt)
    return dmr.make_model(np.array([-1, 0], np.int32), np.array([[0, 0, 0], [0.3, -0.2, 0.5]], np.float32))


def inputs(model, B, seed):
    """Angles within +-1.5 rad, joint velocities ~ N(0, 3), root twist ~ N(0, 2), unit roots (float32)."""
    rng = np.random.default_rng(seed)
    nd = len(model["parents"]) - 1
    q = rng.normal(size=(B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return (rng.uniform(-1.5, 1.5, (B, nd)).astype(np.float32), rng.normal(0, 3, (B, nd)).astype(np.float32),
            q.astype(np.float32), rng.normal(0, 0.5, (B, 3)).astype(np.float32), rng.normal(0, 2, (B, 6)).astype(np.float32))


def twist_error(got, want):
    return np.maximum(ref.frame_error(got[..., :3], want[..., :3]), ref.frame_error(got[..., 3:], want[..., 3:]))


@pytest.mark.parametrize("name", list(BOUNDS))
def test_restatement_against_the_float64_tangent(name):
    B, measured, bound = BOUNDS[name]
    m = tree(name)
    a, ad, q, t, tw = inputs(m, B, 40 + B)
    _, _, got = ref.link_twists(m, a, ad, q, t, tw)
    want = ref.central_twists64(m, a, ad, q, t, tw)
    # the float64 rule is the tangent: its own distance to the differences is the differences' error
    _, _, exact = ref.link_twists64(m, a, ad, q, t, tw)
    own = float(twist_error(exact, want).max())
    err = float(twist_error(got, want).max())
    assert bound == pytest.approx(4 * measured, rel=1e-3)
    print(f"{name}: float32 restatement vs float64 central differences {err:.3e} (measured {measured}, bound {bound}); "
          f"float64 rule vs the differences {own:.3e}")
    assert own < 1e-8
    assert got.dtype == np.float32 and err <= bound


@pytest.mark.parametrize("name", list(BOUNDS))
def test_clip_rule_against_differences_of_the_clamped_model(name):
    """Strictly inside the limits the joint turns, strictly outside it does not: central differences of the clamped
    float64 model.  Exactly at a limit the rule keeps the rate: the derivative of the clamped pose toward the inside,
    taken as the one-sided second-order difference with every rate pointing inward."""
    m = tree(name)
    B = 96
    a, ad, q, t, tw = inputs(m, B, 7)
    nd = a.shape[1]
    rng = np.random.default_rng(3)
    lo, hi = m["lower"], m["upper"]
    gap = 1e-3   # the differences move the angles by |ad| h ~ 1e-5: the frames stay on their side
    kind = rng.integers(0, 3, (B, nd))
    inside = (lo + gap + (hi - lo - 2 * gap) * rng.uniform(0, 1, (B, nd))).astype(np.float32)
    outside = np.where(rng.integers(0, 2, (B, nd)) == 0, lo - gap - rng.uniform(0, 1, (B, nd)),
                       hi + gap + rng.uniform(0, 1, (B, nd))).astype(np.float32)
    a = np.where(kind == 0, outside, inside)
    assert ((a > lo) & (a < hi))[kind != 0].all() and ((a < lo) | (a > hi))[kind == 0].all() and (kind == 0).sum() > nd
    want = ref.central_twists64(m, a, ad, q, t, tw, clip=True)
    _, _, got64 = ref.link_twists64(m, a, ad, q, t, tw, clip=True)
    assert twist_error(got64, want).max() < 1e-8
    _, _, got = ref.link_twists(m, a, ad, q, t, tw, clip=True)
    assert twist_error(got, want).max() < 1e-5
    s = ref.rates(a, ad, lo, hi, True)
    assert (s[kind == 0] == 0).all() and not np.signbit(s[kind == 0]).any() and (s[kind != 0] == ad[kind != 0]).all()
    # exactly at a limit, every rate pointing inward: the clamped model is smooth on [0, 2h]
    at = np.where(rng.integers(0, 2, (B, nd)) == 0, lo, hi).astype(np.float32)
    ad_in = np.where(at == lo, np.abs(ad), -np.abs(ad)).astype(np.float32)
    assert ((at == lo) | (at == hi)).all()
    np.testing.assert_array_equal(ref.rates(at, ad_in, lo, hi, True), ad_in)          # the rule keeps the rate
    h = 1e-5
    P = [ref.dof_fk64(m, *ref.advance64(m, at, ad_in, q, t, tw, k * h), True)[1] for k in (0, 1, 2)]
    v_in = (-3 * P[0] + 4 * P[1] - P[2]) / (2 * h)
    _, _, got64 = ref.link_twists64(m, at, ad_in, q, t, tw, clip=True)
    assert ref.frame_error(got64[..., :3], v_in).max() < 1e-6
    if nd > 1:   # and the other way the joint is held: the inward difference tells the two apart
        _, _, held = ref.link_twists64(m, at, np.zeros_like(ad_in), q, t, tw, clip=True)
        assert ref.frame_error(held[..., :3], v_in).max() > 1e-3


@pytest.mark.parametrize("name", list(BOUNDS))
def test_adjoint_identity_with_the_models_autograd(name):
    """sum_j <c_j, v_j> = <J^T c, ad>: the rule's linear velocities (float64, zero root twist) against the float64
    autograd of the model's positions -- the Jacobian rtg_dof_fk_backward_f32 transposes."""
    import torch
    m = tree(name)
    B = 64
    a, ad, q, t, _ = inputs(m, B, 19)
    J = len(m["parents"])
    c = np.random.default_rng(2).normal(size=(B, J, 3))

    def qmul(x, y):
        ax, ay, az, aw = x.unbind(-1)
        bx, by, bz, bw = y.unbind(-1)
        return torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                            aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)

    at = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    G, P = [torch.tensor(q, dtype=torch.float64)], [torch.tensor(t, dtype=torch.float64)]
    conj = torch.tensor([-1.0, -1.0, -1.0, 1.0], dtype=torch.float64)
    for j in range(1, J):
        p, ax = int(m["parents"][j]), int(m["axis"][j - 1])
        e = torch.zeros(B, 4, dtype=torch.float64)
        lq = e.index_put((torch.arange(B), torch.full((B,), ax)), torch.sin(at[:, j - 1] / 2))
        lq = lq.index_put((torch.arange(B), torch.full((B,), 3)), torch.cos(at[:, j - 1] / 2))
        g = qmul(G[p], lq)
        G.append(g / g.norm(dim=-1, keepdim=True))
        lt = torch.cat([torch.tensor(m["local_t"][j], dtype=torch.float64), torch.zeros(1, dtype=torch.float64)]).expand(B, 4)
        P.append(qmul(qmul(G[p], lt), G[p] * conj)[:, :3] + P[p])
    Pt = torch.stack(P, 1)
    G64, P64, tw = ref.link_twists64(m, a, ad, q, t, None)
    np.testing.assert_allclose(Pt.detach().numpy(), P64, rtol=0, atol=1e-12)       # one model, written twice
    if J == 2:   # the one joint's angle moves no position: both sides are zero
        assert not Pt.requires_grad and (tw[..., :3] == 0).all()
        return
    (Jtc,) = torch.autograd.grad((Pt * torch.tensor(c)).sum(), at)
    lhs = (c * tw[..., :3]).sum((1, 2))
    rhs = (Jtc.numpy() * ad.astype(np.float64)).sum(1)
    np.testing.assert_allclose(lhs, rhs, rtol=1e-11, atol=1e-11 * np.abs(rhs).max())
    assert np.abs(rhs).max() > 1


# ------------------------------------------------------------------------------------------- the entries' checks
def _lib():
    from rtg import _lib as L
    return L, L.lib()


P0, ODD = 0x10000, 0x10008   # fake device addresses: every check below comes before any use


def _p(x):
    return None if x is None else ctypes.c_void_p(x)


def test_dof_fk_vel_rejections_need_no_device():
    L, lib = _lib()
    assert lib.rtg_abi_version() == 7
    assert hasattr(lib, "rtg_dof_fk_vel_f32") and "rtg_dof_fk_vel_f32" in L.SIGNATURES

    def call(dof=P0, rr=P0 + 0x1000, rt=P0 + 0x2000, dv=P0 + 0x3000, rv=None, B=4, clip=0, gr=P0 + 0x5000,
             gp=P0 + 0x6000, gv=P0 + 0x7000):
        rc = lib.rtg_dof_fk_vel_f32(None, _p(dof), _p(rr), _p(rt), _p(dv), _p(rv), B, clip, _p(gr), _p(gp), _p(gv), None)
        return rc, lib.rtg_last_error().decode()

    for kw, word in ((dict(B=-1), "B=-1"), (dict(gv=None), "NULL buffer"), (dict(rr=None), "NULL buffer"),
                     (dict(rt=None), "NULL buffer"), (dict(gr=None), "both g_rot and g_pos"),
                     (dict(gp=None), "both g_rot and g_pos"), (dict(rr=ODD), "aligned"), (dict(gr=ODD), "aligned"),
                     (dict(), "NULL model"), (dict(B=0), "NULL model"), (dict(gr=None, gp=None), "NULL model"),
                     (dict(rv=P0 + 0x8000, clip=1), "NULL model")):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("rtg_dof_fk_vel_f32: ") and word in msg, (kw, rc, msg)


def test_dof_motion_sample_vel_rejections_need_no_device():
    L, lib = _lib()
    assert hasattr(lib, "rtg_dof_motion_sample_vel_f32") and "rtg_dof_motion_sample_vel_f32" in L.SIGNATURES
    fn = lib.rtg_dof_motion_sample_vel_f32
    GV, KV, KP = P0 + 0xD000, P0 + 0xE000, P0 + 0xA000

    def call(N=4, flags=0, keys=None, K=None, dv=P0 + 0x8000, rv=P0 + 0x9000, gr=None, gp=None, kp=None, gv=None,
             kv=None, rro=P0 + 0x6000):
        ka = None if keys is None else np.asarray(keys, np.int32)
        kptr = None if ka is None else ka.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        rc = fn(None, None, _p(P0), _p(P0 + 0x1000), _p(P0 + 0x2000), _p(P0 + 0x3000), _p(P0 + 0x4000), N, flags, kptr,
                (0 if ka is None else len(ka)) if K is None else K, _p(P0 + 0x5000), _p(dv), _p(rro), _p(P0 + 0x7000),
                _p(rv), _p(gr), _p(gp), _p(kp), _p(gv), _p(kv), None)
        return rc, lib.rtg_last_error().decode()

    new = "rtg_dof_motion_sample_vel_f32: "
    for kw, word in ((dict(gv=GV, N=-1), "N=-1"), (dict(gv=GV, flags=4), "unknown flags 0x4"),
                     (dict(gv=GV, K=33, keys=[0] * 33, kp=KP), "K=33"),
                     (dict(gv=GV, keys=[0, 64], kv=KV), "key_links[1]=64"),
                     (dict(gv=GV, rv=None, dv=None), "need dof_vel_out and root_vel_out"),
                     (dict(kv=KV, keys=[1], rv=None, dv=None), "need dof_vel_out and root_vel_out"),
                     (dict(gv=GV, rv=None), "dof_vel_out"),
                     (dict(kv=KV), "go with K > 0"),                               # key_vel without key links
                     (dict(gv=GV, keys=[1, 2]), "go with K > 0"),                   # key links without key_pos / key_vel
                     (dict(gv=GV, gr=P0 + 0xB000), "both g_rot and g_pos"),
                     (dict(gv=GV, rro=ODD), "aligned"),
                     (dict(gv=GV), "NULL model"), (dict(kv=KV, keys=[0, 0, 63]), "NULL model"),
                     (dict(gv=GV, kv=KV, keys=[5], kp=KP, gr=P0 + 0xB000, gp=P0 + 0xC000, flags=3), "NULL model"),
                     (dict(gv=GV, N=0), "NULL model")):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(new) and word in msg, (kw, rc, msg)
    # with both new outputs NULL the call is rtg_dof_motion_sample_f32, its messages under its name
    old = "rtg_dof_motion_sample_f32: "
    for kw, word in ((dict(), "NULL model"), (dict(keys=[1, 2]), "key_pos goes with K > 0"), (dict(kp=KP), "key_pos"),
                     (dict(rv=None), "dof_vel_out"), (dict(flags=8), "unknown flags 0x8")):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(old) and word in msg, (kw, rc, msg)


# ------------------------------------------------------------------------------------------- the Python keywords
def test_python_keywords_validate_without_a_gpu():
    import torch
    import rtg.motion as M
    from rtg import ops
    from robot_kinematics_model.hu_forward_model import HuForwardModel
    assert ops.DofMotionSampleResult._fields[-2:] == ("g_vel", "key_vel")
    r = ops.DofMotionSampleResult(*range(8))                                        # the positional form of before
    assert r.g_vel is None and r.key_vel is None and r.key_pos == 7
    s = M.DofMotionSample(1, 2, 3)
    assert (s.global_velocity, s.global_angular_velocity, s.key_velocity, s.key_angular_velocity) == (None,) * 4
    assert M.DofMotionSample(*range(9)).key_translation == 8
    model = types.SimpleNamespace(num_dofs=3, has_limits=False)
    z = torch.zeros(4, 3)
    for kw in (dict(want_link_velocity=True), dict(want_key_velocity=True, key_links=[1])):
        with pytest.raises(ValueError, match="need want_velocity"):
            ops.dof_motion_sample(model, None, z, z, z, [0], [0.0], want_velocity=False, **kw)
    for keys in (None, []):
        with pytest.raises(ValueError, match="needs key_links"):
            ops.dof_motion_sample(model, None, z, z, z, [0], [0.0], want_key_velocity=True, key_links=keys)
    with pytest.raises(ValueError, match="limits"):
        ops.dof_link_velocity(model, z, torch.zeros(4, 4), z, z, clip=True)
    ml = M.DofMotionLibrary.__new__(M.DofMotionLibrary)
    ml.model, ml.node_names = model, []
    with pytest.raises(ValueError, match="link_velocities needs want_velocity"):
        ml.sample([0], [0.0], link_velocities=True, want_velocity=False)
    hu = HuForwardModel.__new__(HuForwardModel)
    hu._model = model
    with pytest.raises(ValueError, match="limits"):
        hu.link_velocities(z, z, torch.zeros(4, 1, 4), z, clip_angles=True)

"""The hostile sequences and frames of tests/kinematics_frames.py on the host: the C oracle against the reference's own
outputs for them (tests/golden/motion_adversarial.npz and kinematics_adversarial.npz, recorded by tools/make_golden.py)
and the oracle-only conditions the GPU tests (tests/test_gpu_motion_hostile.py, tests/test_gpu_kinematics_hostile.py)
rest on.

FK, inverse FK, their SkeletonState forms and the linear velocity: bit for bit, NaN-aware and sign-of-zero-aware
(retarget_to_ref.bits).  Angular velocity: the same NaN / inf / zero / sign pattern, finite values within 4 ulp of
float32(pi) / float32(dt) -- the reference takes torch's acos, the oracle a correctly rounded one."""
import zlib

import numpy as np
import pytest

from conftest import golden

import kinematics_frames as kf
import oracle as orc
from retarget_to_ref import bits

FPS = (30, 120)
CONJ = np.float32([-1, -1, -1, 1])


def _taps():
    from scipy.ndimage._filters import _gaussian_kernel1d
    return np.ascontiguousarray(_gaussian_kernel1d(2, 0, 8)[::-1])


@pytest.mark.parametrize("name", ["hu_v5", "vtrdyn_full"])
def test_fk_family_matches_the_recorded_reference(name):
    """cal_forward_kinematics, cal_local_rotation, SkeletonState FK and local_rotation on the 18 quaternion families, 8
    frames each (unit, non-unit, near-unit, negated, identity, half turns, gimbal, w edges, scales 1e-40 .. 1e18, zero /
    NaN / inf rows, signed zeros): the oracle equals the reference's bits in every family."""
    from rtg import assets
    g = golden("kinematics_adversarial")
    p, lt, tq = assets.parents(name), assets.local_translation(name), assets.tree_quat(name)
    lr, rt, fam = kf.fk_rotations(len(p), 8)
    assert g["families"].tolist() == list(kf.FK_FAMILIES) and len(lr) == 8 * 18
    assert zlib.crc32(lr.tobytes() + rt.tobytes()) == int(g[f"{name}_input_crc"]), "the helper's frames moved: record again"
    B, J = lr.shape[:2]
    with np.errstate(all="ignore"):
        gr, gp = orc.fk(p, lt, lr, rt)
        inv = orc.local_rotation(p, g[f"{name}_g_rot"])
        sr, sp = orc.state_fk(p, tq, lt, orc.quat_normalize(lr.reshape(-1, 4)).reshape(B, J, 4), rt)
        sl = orc.state_local_rotation(p, tq, orc.quat_normalize(g[f"{name}_state_g_rot"].reshape(-1, 4)).reshape(B, J, 4))
    got = {"g_rot": gr, "g_pos": gp, "inv_local": inv, "state_g_rot": sr, "state_g_pos": sp, "state_local_rot": sl}
    for k, fname in enumerate(kf.FK_FAMILIES):
        rows = fam == k
        for key, a in got.items():
            np.testing.assert_array_equal(bits(a[rows]), bits(g[f"{name}_{key}"][rows]), err_msg=f"{name} {fname} {key}")
    nonfinite = ~np.isfinite(g[f"{name}_g_rot"]).all(axis=(1, 2))
    print(f"{name}: {B} frames of {len(kf.FK_FAMILIES)} families bit-equal to the reference in all six outputs "
          f"({int(nonfinite.sum())} frames with NaN / inf global rotations)")
    assert nonfinite.any() and not nonfinite.all()


def test_linear_velocity_matches_the_recorded_reference():
    """np.gradient / dt and gaussian_filter1d on static, ramp, subnormal, overflowing, cancelling, NaN, inf and random
    positions: the oracle equals the reference's bits, smoothed and raw, at both frame rates."""
    g = golden("motion_adversarial")
    w = _taps()
    assert g["pos_families"].tolist() == list(kf.POS_FAMILIES)
    for fam in kf.POS_FAMILIES:
        p = kf.pos_sequence(fam, 40, 8)
        np.testing.assert_array_equal(bits(p), bits(g[f"pos_{fam}"]), err_msg="the helper's sequences moved: record again")
        for fps in FPS:
            for tag, taps in (("smooth", w), ("raw", None)):
                with np.errstate(all="ignore"):
                    v = orc.linear_velocity(p, 1 / fps, taps)
                np.testing.assert_array_equal(bits(v), bits(g[f"lin_{fam}_{fps}_{tag}"]), err_msg=f"{fam} {fps} {tag}")
        print(f"linear {fam}: bit-equal to the reference, smoothed and raw, fps {FPS}")


def test_angular_velocity_matches_the_recorded_reference():
    """Per rotation family, fps and filter: NaN where the reference has NaN, the same infinities, zeros exactly where it
    has zeros, the same sign on every element that is not NaN (the sign of a zero included), and every finite value
    within 4 ulp of float32(pi) / float32(dt): torch's acos within 1 ulp of the angle is up to 2 ulp of the quotient
    across a binade, the product by the axis and the quotient by dt each round once more, one ulp is spare."""
    g = golden("motion_adversarial")
    w = _taps()
    assert g["rot_families"].tolist() == list(kf.ROT_FAMILIES)
    for fam in kf.ROT_FAMILIES:
        r = kf.rot_sequence(fam, 40, 8)
        np.testing.assert_array_equal(bits(r), bits(g[f"rot_{fam}"]), err_msg="the helper's sequences moved: record again")
        worst = 0.0
        for fps in FPS:
            ulp = float(np.spacing(np.float32(np.pi) / np.float32(1 / fps)))
            for tag, taps in (("smooth", w), ("raw", None)):
                with np.errstate(all="ignore"):
                    v = orc.angular_velocity(r, 1 / fps, taps)
                ref = g[f"ang_{fam}_{fps}_{tag}"]
                msg = f"{fam} {fps} {tag}"
                np.testing.assert_array_equal(np.isnan(v), np.isnan(ref), err_msg=msg)
                ok = ~np.isnan(ref)
                np.testing.assert_array_equal(np.isinf(v), np.isinf(ref), err_msg=msg)
                np.testing.assert_array_equal(v[ok] == 0, ref[ok] == 0, err_msg=msg)
                np.testing.assert_array_equal(np.signbit(v[ok]), np.signbit(ref[ok]), err_msg=msg)
                fin = np.isfinite(ref)
                if fin.any():
                    worst = max(worst, float(np.abs(v[fin].astype(np.float64) - ref[fin].astype(np.float64)).max()) / ulp)
        print(f"angular {fam}: pattern equal; max |oracle - reference| = {worst:.3g} ulp of pi / dt")
        assert worst <= 4.0, (fam, worst)


def _pairs(r):
    """The normalised relative rotations d_t = normalize(r[t+1] * conj(r[t])) of a sequence, as the oracle computes them."""
    a = np.ascontiguousarray(r[1:].reshape(-1, 4))
    b = np.ascontiguousarray((r[:-1] * CONJ).reshape(-1, 4))
    with np.errstate(all="ignore"):
        return orc.quat_mul_norm(a, b)


def test_rare_paths_are_reached():
    """From oracle primitives alone, on the shapes the GPU tests use: the near_unit products' squared norms fall on the
    near-unit table (|code| < 16), on its edge (+-16) and off it (+-17 .. 20); dt = 1e30 makes nonzero subnormal
    quotients (the mulr branch) of tiny_step's small dividends and of the subnormal positions, dt = 3e38 of every ordinary
    dividend, and a subnormal dt = 1e-40 overflows them (1e-30 only those above 3.4e8, as in the huge family: an ordinary
    velocity of ~1 divided by 1e30 is 1e-30, a normal float32); tiny_step reaches 2 w^2 - 1 == 1 beside a
    nonzero imaginary part, |xyz|^2 subnormal, |xyz|^2 == 0 beside a nonzero part, and norms on both sides of the 1e-9
    clamp; half_turn reaches w == 0 and |w| < 1e-6, antipodal w == 1 after the sign flip of a negated frame; static the
    exact identity; w_edges every edge value."""
    f32 = np.float32
    c = kf.product_codes(kf.rot_sequence("near_unit", 130, 31))
    assert (np.abs(c) < 16).any() and np.isin(c, (-16, 16)).any() and np.isin(np.abs(c), (17, 18, 19, 20)).any()
    assert (c == 16).any() and (c == -16).any() and (c == 17).any() and (c == -17).any()
    c = kf.product_codes(kf.rot_sequence("smooth", 130, 31))
    assert (np.abs(c) < 16).all()
    # dt = 1e30: a dividend below 1.2e-8 has a subnormal quotient (tiny_step's angles, the subnormal positions, whose
    # quotients round to zero); dt = 3e38 makes every ordinary quotient subnormal
    raw = orc.angular_velocity(kf.rot_sequence("tiny_step", 130, 31), 1.0, None)
    rare, sub = kf.subnormal_quotients(raw, 1e30)
    assert rare > 100 and sub > 100, (rare, sub)
    raw = orc.angular_velocity(kf.rot_sequence("smooth", 130, 31), 1.0, None)
    assert kf.subnormal_quotients(raw, 1e30) == (0, 0) and kf.subnormal_quotients(raw, 3e38)[1] > 1000
    with np.errstate(all="ignore"):
        raw = orc.linear_velocity(kf.pos_sequence("subnormal", 130, 31), 1.0, None)
        assert kf.subnormal_quotients(raw, 1e30)[0] > 1000
        raw = orc.linear_velocity(kf.pos_sequence("random", 130, 31), 1.0, None)
        assert kf.subnormal_quotients(raw, 3e38)[1] > 1000
        # dt = 1e-30 overflows dividends above 3.4e8 only (none here); a subnormal dt = 1e-40 overflows these
        assert not np.isinf(raw / f32(1e-30)).any() and np.isinf(raw / f32(1e-40)).mean() > 0.9
    d = _pairs(kf.rot_sequence("tiny_step", 130, 31))
    xyz2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    part = np.abs(d[:, :3]).max(axis=1)
    cosv = f32(2) * (d[:, 3] * d[:, 3]) - f32(1)
    assert ((cosv == 1) & (part > 0)).any()
    assert ((xyz2 > 0) & (xyz2 < f32(2.0 ** -126))).any() and ((xyz2 == 0) & (part > 0)).any()
    n = np.sqrt(xyz2.astype(np.float64))
    assert ((n > 0) & (n < 1e-9)).any() and ((n >= 1e-9) & (n < 1e-8)).any()
    w = _pairs(kf.rot_sequence("half_turn", 130, 31))[:, 3]
    assert (w == 0).any() and ((w != 0) & (np.abs(w) < 1e-6)).any()
    r = kf.rot_sequence("antipodal", 130, 31)
    raw_w = orc.quat_mul(np.ascontiguousarray(r[1:].reshape(-1, 4)), np.ascontiguousarray((r[:-1] * CONJ).reshape(-1, 4)))[:, 3]
    assert (raw_w < -0.99).mean() > 0.3 and (raw_w > 0.99).mean() > 0.2 and (_pairs(r)[:, 3] == 1).any()
    d = _pairs(kf.rot_sequence("static", 130, 31))
    assert ((d[:, 3] == 1) & (d[:, :3] == 0).all(axis=1)).mean() > 0.5
    w = _pairs(kf.rot_sequence("w_edges", 130, 31))[:, 3]
    for e in kf.W_EDGES:
        assert (np.abs(w) == abs(e)).any(), e


def test_tie_quotients_defeat_a_rounded_reciprocal():
    """The inputs of the GPU tests' tie cases, in host arithmetic: every quotient is an exact tie between two subnormal
    float32 values, the oracle's IEEE division rounds it to even, and the product by RN(1 / n) in float64 -- the kernels'
    shared-reciprocal division without its subnormal branch -- rounds some of them the other way."""
    for n in kf.TIE_DIVISORS[:3]:
        a = kf.midpoint_dividends(n, 93)
        np.testing.assert_array_equal(a.astype(np.float64) / n, (2 * np.arange(93) + 1) * 2.0 ** -150)
        q = a / np.float32(n)
        np.testing.assert_array_equal(q.view(np.uint32) % 2, 0)          # ties to even
        wrong = kf.shortcut_misrounds(a, n)
        print(f"n = {n:g}: the rounded-reciprocal product misrounds {int(wrong.sum())} of {len(a)} ties")
        p = kf.midpoint_ramp(130, 31, n)
        with np.errstate(all="ignore"):
            raw = orc.linear_velocity(p, 1.0, None)
        assert ((np.abs(raw.astype(np.float64)) / n * 2.0 ** 150) % 2 == 1).all()   # every gradient: an odd multiple
        assert kf.shortcut_misrounds(raw, n).mean() > 0.3
    assert not kf.shortcut_misrounds(kf.midpoint_dividends(10.0, 93), 10.0).any()   # RN(1 / 10) is too close
    dt = kf.ANGULAR_TIE_DT
    raw = orc.angular_velocity(kf.angular_tie_sequence(130, 31), 1.0, None)[:-1]
    small = raw[(raw != 0) & (np.abs(raw) < 1)]
    tie = (np.abs(small.astype(np.float64)) / dt * 2.0 ** 150) % 2 == 1
    wrong = kf.shortcut_misrounds(small, dt)
    print(f"angular: {int(tie.sum())} of {small.size} small quotients are ties, {int(wrong.sum())} misrounded by the "
          f"rounded-reciprocal product")
    assert small.size == 129 * 31 and tie.sum() >= 129 * 5 and wrong.sum() >= 129 * 3
    assert (np.abs(raw[np.abs(raw) >= 1]) == np.float32(np.pi)).all()
    q = kf.midpoint_rows(31, 16)[:, 1:]
    n2 = ((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3]
    assert (np.sqrt(n2) == np.abs(q[..., 3])).all()                       # the row's norm is |w| exactly
    assert sum(int(kf.shortcut_misrounds(q[np.abs(q[..., 3]) == W][:, :3], W).any()) for W in kf.MIDPOINT_NORMS) >= 3


def test_host_filter_is_the_oracles():
    """kinematics_frames.gauss_nearest over the oracle's raw velocities equals the oracle's smoothed ones bit for bit
    (both velocities, every family, the reference's radius 8 and radius 4, sequences shorter than the radius)."""
    from rtg import ops
    for sigma in (2.0, 1.0):
        w, _ = ops.gaussian_taps(sigma)
        for L in (1, 2, 9, 40):
            with np.errstate(all="ignore"):
                for fam in kf.ROT_FAMILIES:
                    r = np.stack([kf.rot_sequence(fam, L, 5), kf.rot_sequence(fam, L, 5, seed=1)])
                    np.testing.assert_array_equal(bits(kf.gauss_nearest(orc.angular_velocity(r, 1 / 30, None), w)),
                                                  bits(orc.angular_velocity(r, 1 / 30, w)), err_msg=f"{fam} L={L}")
                for fam in kf.POS_FAMILIES if L > 1 else ():
                    p = kf.pos_sequence(fam, L, 5)
                    np.testing.assert_array_equal(bits(kf.gauss_nearest(orc.linear_velocity(p, 1e-3, None), w)),
                                                  bits(orc.linear_velocity(p, 1e-3, w)), err_msg=f"{fam} L={L}")


def test_builder_is_deterministic_and_places_single_elements():
    assert kf.placements(130) == [0, 1, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80, 95, 96, 111, 112, 127, 128, 129]
    assert kf.placements(2) == [0, 1] and kf.placements(17) == [0, 1, 15, 16]
    for fam in ("nan_single", "zero_row_single", "inf_single"):
        r = kf.rot_sequence(fam, 130, 31)
        bad = ~np.isfinite(r).all(axis=2) | (r == 0).all(axis=2)
        assert bad.sum() == len(kf.placements(130)) and (bad.sum(axis=1)[kf.placements(130)] == 1).all()
        np.testing.assert_array_equal(bits(r), bits(kf.rot_sequence(fam, 130, 31)))
    for fam in ("nan", "inf"):
        p = kf.pos_sequence(fam, 130, 31)
        assert (~np.isfinite(p)).sum() == len(kf.placements(130))
    a, b = kf.fk_rotations(59, 8), kf.fk_rotations(59, 8)
    np.testing.assert_array_equal(bits(a[0]), bits(b[0]))

"""The hostile-input frames of tests/other_solver_frames.py for UPPER_BODY, FULL_BODY_ROT and BODY_ROT on the host:
the conditions the GPU tests (tests/test_gpu_other_solvers.py) rest on, checked on the C oracle alone, and the anchor
of the oracle on those families to the reference's own outputs (tests/golden/other_solvers_adversarial.npz, recorded
by tools/make_golden.py other_solvers_adversarial: the first 8 frames of every family's whole wave)."""
import numpy as np
import pytest

from conftest import golden

import oracle as orc
import other_solver_frames as osf

KINDS = sorted(osf.NAMES)
IDS = [osf.NAMES[k] for k in KINDS]
# tests/test_gpu_parity.py GOLD_BOUNDS[...]["max"]: the reference-vs-oracle residual of the benign golden frames
GOLD_MAX = {"upper_body": 8.64e-5, "full_body_rot": 3.27e-5, "body_rot": 1.2e-7}

# Oracle-vs-reference DOF residual per family, over the recorded frames the reference solves: the measured value
# (beside it) rounded up in the third digit -- the rule above tests/test_gpu_parity.py GOLD_BOUNDS.  Measured against
# the recorded reference, never against the GPU.
ADV_BOUNDS = {
    "upper_body": {
        "torso_rotation": 4.18e-07,   # 4.17233e-07
        "torso_coplanar": 3.3e-06,   # 3.29688e-06
        "torso_collinear": 7.64e-06,   # 7.63126e-06
        "torso_mirrored": 9.39e-07,   # 9.38773e-07
        "torso_zero": 5.89e-07,   # 5.88596e-07
        "torso_duplicated": 5.51,   # 5.50697
        "torso_tiny": 1.58e-06,   # 1.57952e-06
        "torso_large": 2.39e-07,   # 2.38419e-07
        "torso_signed_zero": 1.94e-06,   # 1.93343e-06
        "torso_zero_plane": 4.77e-07,   # 4.76837e-07
        "zero_length": 1.79e-07,   # 1.78814e-07
        "axis_arm": 2.39e-07,   # 2.38419e-07
        "straight_elbow": 3.52,   # 3.51097
        "folded_elbow": 1.04,   # 1.03779
        "pscale_1e-30": 0.0,   # 0
        "pscale_1e-12": 2.69e-07,   # 2.68221e-07
        "pscale_1e+12": 1.2e-07,   # 1.19209e-07
        "pscale_1e+25": 0.0,   # 0
        "negzero_torso": 1.79e-07,   # 1.78814e-07
        "nan_arm": 1.2e-07,   # 1.19209e-07
        "inf_arm": 1.2e-07,   # 1.19209e-07
        "negzero_arm": 1.54e-06,   # 1.53482e-06
    },
    "full_body_rot": {
        "unit": 4.77e-07,   # 4.76837e-07
        "nonunit": 8.95e-07,   # 8.9407e-07
        "near_unit": 2.09e-07,   # 2.08616e-07
        "negated": 1.47e-06,   # 1.46776e-06
        "identity": 3.58e-07,   # 3.57628e-07
        "relative_identity": 2.99e-07,   # 2.98023e-07
        "half_turn": 1.76e-06,   # 1.75834e-06
        "gimbal": 0.0966,   # 0.0965288
        "w_table_edges": 8.8e-07,   # 8.79169e-07
        "scale_1e8": 1.8e-06,   # 1.79932e-06
        "scale_1e18": 2.39e-07,   # 2.38419e-07
        "signed_zero": 8.54e-07,   # 8.53091e-07
        "axis_arm": 3.8e-07,   # 3.7998e-07
        "straight_elbow": 0.0253,   # 0.0252614
        "folded_elbow": 1.54,   # 1.53892
        "pscale_1e-12": 1.79e-07,   # 1.78814e-07
        "pscale_1e+12": 6e-06,   # 5.99027e-06
        "pscale_1e+25": 1.2e-07,   # 1.19209e-07
        "negzero_arm": 2.99e-07,   # 2.98023e-07
        "gripper_threshold": 1.2e-07,   # 1.19209e-07
    },
    "body_rot": {
        "unit": 2.39e-07,   # 2.38419e-07
        "nonunit": 5.97e-08,   # 5.96046e-08
        "near_unit": 5.97e-08,   # 5.96046e-08
        "negated": 1.2e-07,   # 1.19209e-07
        "identity": 0.0,   # 0
        "relative_identity": 5.97e-08,   # 5.96046e-08
        "half_turn": 5.97e-08,   # 5.96046e-08
        "gimbal": 4.77e-07,   # 4.76837e-07
        "w_table_edges": 1.2e-07,   # 1.19209e-07
        "scale_1e-12": 2.99e-08,   # 2.98023e-08
        "scale_1e-20": 5.97e-08,   # 5.96046e-08
        "scale_1e8": 5.97e-08,   # 5.96046e-08
        "signed_zero": 5.97e-08,   # 5.96046e-08
    },
}
# the families whose bound is more than 10x the kind's GOLD_MAX, each explained in
# test_oracle_matches_the_recorded_reference's docstring
ILL_POSED = {"upper_body": {"torso_duplicated", "straight_elbow", "folded_elbow"},
             "full_body_rot": {"gimbal", "straight_elbow", "folded_elbow"}, "body_rot": set()}


@pytest.fixture(scope="module")
def solved():
    """Per kind: the N0 frames and the oracle's dof, local_rot and status for them, computed once."""
    out = {}
    for kind in KINDS:
        d = osf.frames(kind)
        dof, lr = osf.oracle_run(kind, d)
        out[kind] = dict(d=d, dof=dof, lr=lr, status=orc.frame_status(dof))
    return out


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_layout_and_inputs(kind):
    """N0 distinct deterministic frames: a mixed head that holds every family, one whole wave per family, plain
    frames after them."""
    d = osf.frames(kind)
    nf = len(osf.FAMILIES[kind])
    assert all(d[k].shape[0] == osf.N0 and d[k].dtype == np.float32 for k in osf.INPUTS[kind])
    assert set(d["family"][:osf.HEAD].tolist()) == set(range(nf))
    for k, (name, _, _) in enumerate(osf.FAMILIES[kind]):
        w = osf.wave(kind, name)
        assert len(w) == 64 and w[0] % 64 == 0 and (d["family"][w] == k).all()
    assert (d["family"][osf.HEAD + 64 * nf:] == -1).all() and osf.HEAD + 64 * nf < osf.N0
    flat = np.concatenate([d[k].reshape(osf.N0, -1) for k in osf.INPUTS[kind]], axis=1)
    ordinary = d["family"] < 0
    assert len(np.unique(flat[ordinary].view(np.uint32), axis=0)) == int(ordinary.sum())
    osf._CACHE.pop(kind)
    again = osf.frames(kind)   # a fresh build gives the same bits
    for k in osf.INPUTS[kind]:
        np.testing.assert_array_equal(again[k].view(np.uint32), d[k].view(np.uint32))


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_oracle_conditions_the_gpu_tests_rest_on(solved, kind):
    """The oracle alone: at most 25 % of the frames raise; the only codes are 1 (UPPER_BODY: a NaN / inf torso point
    in the Kabsch matrix) and 2 (a zero-norm quaternion at scipy's from_quat); every family raises on all of its
    whole-wave frames or leaves at least 48 of the 64 solved, as FAMILIES labels it; a status-0 frame has finite DOFs
    in the families FAMILIES lists as finite; a raising frame is all NaN; the plain frames never raise."""
    s = solved[kind]
    st, dof, lr, fam = s["status"], s["dof"], s["lr"], s["d"]["family"]
    assert (st > 0).mean() <= 0.25
    assert set(np.unique(st).tolist()) <= ({0, 1} if kind == osf.UPPER_BODY else {0, 2})
    assert np.isnan(dof[st > 0]).all() and np.isnan(lr[st > 0]).all()
    assert (st[fam < 0] == 0).all() and np.isfinite(dof[fam < 0]).all()
    seen = set()
    for name, raises, finite in osf.FAMILIES[kind]:
        w = osf.wave(kind, name)
        n = int((st[w] > 0).sum())
        assert raises in ("all", "few")
        assert (n == 64) if raises == "all" else (n <= 16), (name, n)
        if finite:
            everywhere = np.flatnonzero((fam == fam[w[0]]) & (st == 0))
            assert np.isfinite(dof[everywhere]).all(), name
        seen.add(raises)
    assert seen == {"all", "few"}


def test_rare_paths_are_reached():
    """The inputs land where they are meant to (host arithmetic on the float32 rows): near_unit squared norms fall on,
    at the edge of and outside the 33 codes around 1.0f; relative_identity wrists give the Euler split a quaternion with
    zero imaginary parts; the gripper frames hit 0.7f and both of its float32 neighbours exactly."""
    f32 = np.float32
    q = osf.frames(osf.BODY_ROT)["global_rot"][osf.wave(osf.BODY_ROT, "near_unit")][:, 13:21]
    n2 = ((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3]
    code = n2.view(np.int32).astype(np.int64) - 0x3F800000
    assert (np.abs(code) <= 16).any() and (code > 16).any() and (code < -16).any()
    assert np.isin(code, (-17, -16, 16, 17)).any()
    d = osf.frames(osf.FULL_BODY_ROT)
    w = osf.wave(osf.FULL_BODY_ROT, "relative_identity")
    zero_imag = 0
    for i in w[:12]:
        for side, row in ((0, 20), (1, 16)):
            par = osf.full_body_rot_wrist_parent(d["body_rot"][i], d["body_pos"][i], d["lh"][i], d["rh"][i], side)
            loc = orc.quat_mul(par.astype(f32)[None] * f32([-1, -1, -1, 1]), d["body_rot"][i, row][None])[0]
            zero_imag += int((loc[:3] == 0).all())
    assert zero_imag >= 12
    orig = osf.gripper_orig()
    hit = set()
    for t in osf.GRIPPER_TARGETS[:3]:
        x = osf._gripper_x(t)
        m = f32(f32(f32(f32(f32(x + x) + x) + x) + x) / f32(5.0))
        hit.add(f32(m / orig) == t)
    assert hit == {True}


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_oracle_matches_the_recorded_reference(solved, kind):
    """The reference itself ran the first 8 frames of every family (tools/make_golden.py other_solvers_adversarial).
    Per family: the oracle raises exactly where the reference raised, with the same code; where the reference solved
    the frame the oracle's DOFs are NaN where its DOFs are, and within ADV_BOUNDS of them.

    Six families exceed ten times the benign frames' bound (GOLD_MAX); in each the reference's own answer is an
    amplification of its last-bit rounding, because the quantity asked for is undetermined by the input:
      * straight_elbow, folded_elbow (UPPER_BODY 3.52 / 1.04 rad, FULL_BODY_ROT 0.0253 / 1.54 rad): the forearm is
        parallel or antiparallel to the upper arm, the arm's kinematic singularity.  cal_elbowP_and_shoulderY projects
        the forearm into the plane across the upper arm and normalises a projection whose length is rounding noise, so
        the shoulder yaw (DOFs 13 / 22) and what is chained on it are the direction of that noise; the reference's
        MKL VML sin / cos / acos / sqrt differ from correctly rounded ones by an ulp there.
        The differing DOFs are only those of the yaw link and, in FULL_BODY_ROT, the wrist x angle that undoes it.
      * gimbal (FULL_BODY_ROT 0.0966 rad): the wrist's XYZ split with the middle angle 1e-8 to 1e-4 off +-pi / 2 sees
        normalize(par * chain), which carries the arm maps' VML noise of ~1e-7; the first and third angles are determined
        only in their sum or difference, and the noise reaches each divided by the distance from the lock (their
        sum keeps to 1e-6: DOFs 24 and 26 move by equal and opposite amounts).  BODY_ROT's gimbal family, whose split
        sees the input rows through exact arithmetic only, stays within 4.77e-7.
      * torso_duplicated (UPPER_BODY 5.51 rad): torso points 17 and 13 coincide (in some frames 11 too).  Their zero
        vectors mirror each other in y and all three have x = 0, so the Kabsch matrix has two exactly zero columns
        and rank one.  Its singular values are (s, 0, 0) in the oracle's restated sgesdd and in MKL's alike, to the
        bit; the singular vectors of the double zero are any orthonormal basis of a plane, and in 7 of the 8
        recorded frames MKL returns the restatement's two vectors in the other order or another basis of that plane.
        Either is an SVD of the matrix and either rotation fits the coinciding points equally; 3 of the 8 frames
        still agree to 1.2e-7.  The device follows the oracle bit for bit (tests/test_gpu_other_solvers.py), so on
        such a frame -- a torso collapsed onto its spine -- this port returns another of the equally good torso
        rotations than the reference does."""
    name = osf.NAMES[kind]
    g = golden("other_solvers_adversarial")
    s = solved[kind]
    idx = g[f"{name}_frame"]
    fams = [f[0] for f in osf.FAMILIES[kind]]
    assert g[f"{name}_family"].tolist() == [f for f in fams for _ in range(8)]
    for k in osf.INPUTS[kind]:   # the recorded inputs are the helper's frames
        np.testing.assert_array_equal(osf._f32(g[f"{name}_{k}"]).view(np.uint32), s["d"][k][idx].view(np.uint32))
    np.testing.assert_array_equal(s["status"][idx], g[f"{name}_status"])
    ref, dof, st = g[f"{name}_dof"], s["dof"][idx], g[f"{name}_status"]
    bounds = dict(ADV_BOUNDS[name])
    for f, (_, raises, _) in zip(fams, osf.FAMILIES[kind]):
        rows = np.flatnonzero((g[f"{name}_family"] == f) & (st == 0))
        assert (len(rows) == 0) == (raises == "all"), f
        if len(rows) == 0:
            assert f not in bounds, f
            continue
        np.testing.assert_array_equal(np.isnan(dof[rows]), np.isnan(ref[rows]), err_msg=f)
        res = float(np.nanmax(np.abs(dof[rows].astype(np.float64) - ref[rows].astype(np.float64))))
        print(f"{name} {f}: oracle-vs-reference DOF residual {res:.6g} (bound {bounds[f]:g})")
        assert res <= bounds.pop(f), (f, res)
    assert not bounds
    loose = {f for f, b in ADV_BOUNDS[name].items() if b > 10 * GOLD_MAX[name]}
    assert loose == ILL_POSED[name]


def _rotmat(q):
    x, y, z, w = (np.float64(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_collapsed_torso_fits_are_equally_good():
    """What exempts torso_duplicated in ILL_POSED, asserted on the recorded frames: the Kabsch matrix M^T Z has two
    exactly zero columns and rank one, so its singular values are (s, 0, 0) and the fit's objective
    sum_i M_i . (R Z_i) is at most s for any rotation; the oracle's torso rotation and the one the reference itself
    returned (recorded as kabsch_q) both reach s to 1e-6 of it -- two equally good fits -- although in most frames
    they are different rotations."""
    g = golden("other_solvers_adversarial")
    rows = np.flatnonzero(g["upper_body_family"] == "torso_duplicated")
    Z = osf.zero_pose()["vtrdyn_local_t"][[17, 13, 11]]
    differ = 0
    for i in rows:
        s = g["upper_body_x"][i] * np.float32([-1, -1, 1])
        M = s[[17, 13, 11]] - s[10]
        A = M.astype(np.float64).T @ Z.astype(np.float64)
        assert (A[:, :2] == 0).all() and np.linalg.matrix_rank(A) == 1
        _, S, _ = orc.sgesdd3((M.T @ Z)[None])
        assert S[0, 0] > 0 and (S[0, 1:] == 0).all()
        top = np.linalg.norm(A[:, 2])
        fits = []
        for q in (orc.cal_joint_quat(Z[None], M[None])[0], g["upper_body_kabsch_q"][i]):
            R = _rotmat(q / np.linalg.norm(q.astype(np.float64)))
            fits.append(float(np.einsum("ij,ij->", M.astype(np.float64), Z.astype(np.float64) @ R.T)))
        assert abs(fits[0] - top) <= 1e-6 * top and abs(fits[1] - top) <= 1e-6 * top, (i, fits, top)
        qo, qr = orc.cal_joint_quat(Z[None], M[None])[0], g["upper_body_kabsch_q"][i]
        differ += int(min(np.abs(qo - qr).max(), np.abs(qo + qr).max()) > 1e-3)
    assert len(rows) == 8 and differ >= 4

"""la_bdsqr3's sweep loop (csrc/rtg_math.cuh: one structured loop, U / VT / d / e held in chase order), bit for bit
against the oracle on inputs that force each of its paths: both chase directions (whole waves and lane by lane),
deflation, the split, each convergence test on and about its threshold, zero-shift and shifted sweeps, lanes of one
wave needing different numbers of sweeps, NaN / inf lanes, SGESDD's rescaling -- through rtg_cal_joint_quat_f32 on
bidiagonal A (tests/sweep_loop_cases.py says how), on 2^20 random dense fits, and through the FULL_BODY_POS solver in
both layouts.  NaNs compare as NaN (tests/test_gpu_torso_fit.py's rule)."""
import numpy as np
import pytest
import torch

from conftest import golden
import sweep_loop_cases as slc

WRIST_JOINTS = (2, 6, 10, 14, 17)
LEFT_Z, RIGHT_Z = (16, 20, 24, 28, 32), (41, 45, 49, 53, 56)
NSOLVE = 129


def _bits(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


@pytest.fixture(scope="module")
def bidiag():
    import oracle as orc
    de, labels = slc.bidiag_frames()
    Z, M = slc.bidiag_points(de)
    return Z, M, orc.cal_joint_quat(Z, M), labels


def test_cases_sit_where_they_claim():
    """On the CPU: the restated thresholds put the named cases on the side they name, every chase case has
    |D1| > |D3| (so that both placements chase as labelled), and the oracle gives a unit quaternion for every finite
    case."""
    import oracle as orc
    for lab, c in slc.chase_cases():
        assert abs(c[0]) > abs(c[2]), lab
    for lab, c in slc.chase_cases():
        if lab.startswith("conv1"):
            k = int(lab.split("k=")[1])
            assert (abs(c[4]) <= slc.TOL * abs(c[2])) == (k <= 0), lab
        if lab.startswith("conv2"):
            k = int(lab.split("k=")[1])
            assert (abs(c[3]) <= slc.TOL * abs(c[0])) == (k <= 0), lab
            assert abs(c[3]) > slc.thresh(*slc.place(c, False)) and abs(c[3]) > slc.thresh(*slc.place(c, True)), lab
    n_defl = n_split = 0
    for lab, c in slc.index_cases():
        t = slc.thresh(*c)
        n_defl += lab.startswith("e2 about") and abs(c[4]) <= t
        n_split += lab.startswith("e1 about") and abs(c[3]) <= t < abs(c[4])
    assert n_defl >= 8 and n_split >= 8
    de, labels = slc.bidiag_frames()
    assert len(de) % 64 == 0 and len(de) == len(labels)
    Z, M = slc.bidiag_points(de)
    q = orc.cal_joint_quat(Z, M)
    fin = np.isfinite(de).all(axis=1)
    assert np.isfinite(q[fin]).all() and not np.isfinite(q[~fin]).all(axis=1).any()
    assert np.abs(np.linalg.norm(q[fin].astype(np.float64), axis=1) - 1.0).max() < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("B", [64, 65, 130])
def test_bidiagonal_cases_vs_oracle(gpu, bidiag, B):
    """Every case of tests/sweep_loop_cases.py in launches of B fits: whole waves, a wave and a lane, two waves and
    two lanes (so the same case meets different neighbours and lane positions at each B)."""
    from rtg import ops
    Z, M, o, labels = bidiag
    for s in range(0, len(Z), B):
        g = ops.cal_joint_quat(Z[s:s + B], M[s:s + B]).cpu().numpy()
        bad = np.nonzero((_bits(g) != _bits(o[s:s + B])).any(axis=1))[0] + s
        assert bad.size == 0, (B, bad.size, [(int(i), labels[int(i)]) for i in bad[:8]])


@pytest.fixture(scope="module")
def dense():
    rng = np.random.default_rng(1620)
    n = 1 << 20
    out = {}
    for npts in (3, 5):
        Z = (rng.standard_normal((n, npts, 3)) * 0.1).astype(np.float32)
        M = (rng.standard_normal((n, npts, 3)) * 0.1).astype(np.float32)
        out[npts] = (Z, M)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("npts", [3, 5])
def test_random_dense_fits_vs_oracle(gpu, dense, npts):
    """2^20 random dense fits: the sweep loop on ordinary matrices, both chase directions mixed in every wave."""
    import oracle as orc
    from rtg import ops
    Z, M = dense[npts]
    g = ops.cal_joint_quat(Z, M).cpu().numpy()
    o = orc.cal_joint_quat(Z, M)
    bad = np.nonzero((_bits(g) != _bits(o)).any(axis=1))[0]
    assert bad.size == 0, (npts, bad.size, bad[:8])


@pytest.fixture(scope="module")
def solver_frames():
    """NSOLVE golden frames; in two of every three the wrist fits' five points are set so that A = M^T Z is (up to
    rounding: M = pinv(Z)^T T^T in float64, rounded to float32) one of the bidiagonal cases, or hold a NaN / inf at
    lanes 0 and 63 -- among ordinary frames.  The oracle's result is computed once."""
    import oracle as orc
    zp = golden("zero_pose")
    zl = zp["vtrdyn_full_local_t"]
    g = golden("full_body_pos_precise")
    idx = np.arange(NSOLVE) % len(g["body"])
    body, lh, rh = (np.ascontiguousarray(g[k][idx]) for k in ("body", "lh", "rh"))
    de, _ = slc.bidiag_frames()
    de = de[np.isfinite(de).all(axis=1)]
    pick = np.random.default_rng(1629).permutation(len(de))
    ho = slc.hostile_cases()
    for i in range(NSOLVE):
        if i % 3 == 2:
            continue
        for s, (h, zi) in enumerate(((lh, LEFT_Z), (rh, RIGHT_Z))):
            Zh = zl[list(zi)].astype(np.float64)
            assert np.linalg.matrix_rank(Zh) == 3
            d1, d2, d3, e1, e2 = de[pick[(2 * i + s) % len(de)]].astype(np.float64)
            T = np.array([[d1, e1, 0.0], [0.0, d2, e2], [0.0, 0.0, d3]])
            M = (np.linalg.pinv(Zh).T @ T.T).astype(np.float32)
            if i % 64 in (0, 63):
                M[(i + s) % 5, (i // 64 + s) % 3] = ho[(i + 3 * s) % len(ho)][1][(i + s) % 5]
            h[i, 0] = 0.0
            h[i, WRIST_JOINTS, :] = M
    odof, olr, obr = orc.full_body_pos(zl, zp["vtrdyn_full_global_t"], body, lh, rh, True)
    return dict(ins=(body, lh, rh), ref=(odof, olr, obr), status=orc.frame_status(odof))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("B", [65, NSOLVE])
def test_full_body_pos_vs_oracle(gpu, solver_frames, layout, B):
    from rtg import _lib, assets
    from rtg.runtime import Solver, frame_status
    zp = golden("zero_pose")
    S = Solver(_lib.SOLVER_FULL_BODY_POS, zp["vtrdyn_full_local_t"], zp["vtrdyn_full_global_t"],
               assets.parents("vtrdyn_full"), True)
    fr = solver_frames
    dev = [torch.from_numpy(np.ascontiguousarray(a[:B])).cuda() for a in fr["ins"]]
    if layout == "soa":
        dev = [t.permute(1, 2, 0).contiguous() for t in dev]
    dof, lr, br = S.retarget(dev, want_local_rot=True, want_body_rot=True, layout=layout)
    np.testing.assert_array_equal(frame_status(dof).cpu().numpy(), fr["status"][:B], err_msg="status")
    assert (fr["status"][:B] != 0).any() and (fr["status"][:B] == 0).sum() > B // 2
    for name, got, ref in (("dof", dof, fr["ref"][0]), ("local_rot", lr, fr["ref"][1]), ("body_rot", br, fr["ref"][2])):
        bad = np.nonzero((_bits(got.cpu().numpy()) != _bits(ref[:B])).reshape(B, -1).any(axis=1))[0]
        assert bad.size == 0, (layout, B, name, bad.size, bad[:8])

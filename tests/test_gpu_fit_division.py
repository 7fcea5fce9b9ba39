"""The Kabsch fits on point sets whose SVD operands straddle the window of the shared-reciprocal division (fdiv_n,
csrc/rtg_math.cuh: |x| in [2^-47, 2^47]; the issue's first proposal was [2^-40, 2^40], SGESDD's own rescale
thresholds, and both sets of edges are driven here), bit for bit against the oracle: through rtg_cal_joint_quat_f32
with 3 and 5 points, and through the FULL_BODY_POS solver on every kernel route and both input layouts.  NaNs compare
as NaN (tests/test_gpu_torso_fit.py's rule).

Families, per fit:
  scaled      the point set times 2^k so that anrm = max |A| (A = M^T Z) sits at 2^-41 .. 2^-39, 2^39 .. 2^41 (SGESDD
              rescales beyond 2^+-40), at 2^-48 .. 2^-46 and 2^46 .. 2^48 (the division window's edges), at every
              binade between, and far beyond both (2^+-60 .. 2^+-120);
  near_diag   A nearly diagonal: M = Z D + 2^-j noise, j = 10 .. 75 (tiny off-diagonals: tiny g against d in SLARTG);
  near_rank1  A nearly rank 1: collinear points plus 2^-j noise (two tiny singular values, so SLARTG's f and g are
              both tiny: below the window, and below SLARTG's own rtmin);
  zero_line   an exactly zero row of A (a zero coordinate in every M) and, where Z is free, an exactly zero column;
  denormal    all of M denormal, or one denormal entry in an ordinary M;
  hostile     ordinary frames with a NaN / +-inf / 2^+-100 frame at lanes 0 and 63 of a wave.
"""
import numpy as np
import pytest
import torch

from conftest import golden

FAMILIES = ["scaled", "near_diag", "near_rank1", "zero_line", "denormal", "hostile"]
NF = len(FAMILIES)
LATENCY_MAX_B = 49152                    # RTG_LATENCY_MAX_B (checked against the library below)
N0 = 4097                                # distinct frames; a longer batch repeats them
BATCHES = (2, 63, 64, 65, 129, 4097, LATENCY_MAX_B + 1)   # quad8 .. quad, latency5, the side kernel; B = 1 apart
TORSO_JOINTS, WRIST_JOINTS = (17, 13, 11), (2, 6, 10, 14, 17)
TORSO_Z, LEFT_Z, RIGHT_Z = (11, 36, 34), (16, 20, 24, 28, 32), (41, 45, 49, 53, 56)
# anrm exponents of the scaled family: around both rescale thresholds and both window edges, between, and far out
SCALE_EXPS = list(range(-50, -36)) + list(range(37, 51)) + [-120, -100, -80, -60, -30, -10, 0, 10, 30, 60, 80, 100, 120]


def _bits(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def _rand_rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _family_points(fam, Z, i, rng):
    """An (n, 3) float32 point set M of the family for the zero vectors Z (n, 3); i picks the family's variant."""
    n = len(Z)
    Zd = Z.astype(np.float64)
    good = Zd @ _rand_rot(rng).T + rng.normal(0.0, 1e-3, (n, 3))
    if fam == "scaled":
        e = SCALE_EXPS[i % len(SCALE_EXPS)]
        anrm = np.abs(good.astype(np.float32).astype(np.float64).T @ Zd).max()
        M = np.ldexp(good.astype(np.float32), int(e - np.floor(np.log2(anrm))))   # exact: anrm scales with it
    elif fam == "near_diag":
        M = Zd * rng.uniform(0.5, 2.0, 3) + np.ldexp(rng.normal(size=(n, 3)), -(10 + i % 66))
    elif fam == "near_rank1":
        M = 0.3 * rng.normal(size=(n, 1)) * rng.normal(size=3) + np.ldexp(rng.normal(size=(n, 3)), -(10 + i % 66))
        if i % 3 == 0:
            M = 0.3 * rng.normal(size=(n, 1)) * np.eye(3)[(i // 3) % 3] + np.ldexp(rng.normal(size=(n, 3)), -(30 + i % 40))
    elif fam == "zero_line":
        M = good.copy()
        M[:, i % 3] = [0.0, -0.0][(i // 3) % 2]
        if (i // 6) % 2:
            M[:, (i + 1) % 3] = 0.0
    elif fam == "denormal":
        if i % 2:
            M = np.ldexp(good, -140 - i % 8)
        else:
            M = good.copy()
            M[rng.integers(n), rng.integers(3)] = rng.choice([1e-40, -1e-40, 1.4e-45, 1e-38])
    elif fam == "hostile":
        M = good
    else:
        raise KeyError(fam)
    return np.asarray(M, np.float64).astype(np.float32)


def _make_hostile(M, i, rng):
    """Frame i of a hostile wave: lanes 0 and 63 get a NaN / inf / out-of-window point set."""
    if i % 64 not in (0, 63):
        return M
    M = M.copy()
    kind = (i // 64 + (i % 64 == 63)) % 4
    if kind == 0:
        M[rng.integers(len(M)), rng.integers(3)] = np.nan
    elif kind == 1:
        M[rng.integers(len(M)), rng.integers(3)] = rng.choice([np.inf, -np.inf])
    else:
        M = np.ldexp(M, 100 if kind == 2 else -100)
    return M


def _family_of(i):
    """Whole 64-frame waves of one family (the kernels' rare-case branches are decided per wave), then mixed."""
    return (i // 64) % NF if i < 64 * 4 * NF else i % NF


@pytest.fixture(scope="module")
def kabsch_sets():
    """(Z, M) batches for cal_joint_quat with 3 and 5 points, Z free (random per frame), and the oracle's result."""
    import oracle as orc
    rng = np.random.default_rng(1313)
    out = {}
    for npts in (3, 5):
        n = 8192 + 65
        Z = (rng.standard_normal((n, npts, 3)) * 0.1).astype(np.float32)
        M = np.empty_like(Z)
        for i in range(n):
            fam = FAMILIES[_family_of(i)]
            if fam == "zero_line" and (i // 12) % 2:
                Z[i, :, (i + 2) % 3] = 0.0                       # an exactly zero column of A
            M[i] = _family_points(fam, Z[i], i // NF if i >= 64 * 4 * NF else i, rng)
            if fam == "hostile":
                M[i] = _make_hostile(M[i], i, rng)
        out[npts] = (Z, M, orc.cal_joint_quat(Z, M))
    return out


@pytest.fixture(scope="module")
def fit_frames():
    """N0 golden frames with the three fits' points overwritten by the families, repeated up to the side kernel's
    smallest batch, and the oracle's result for them (computed once on the N0: frames are independent)."""
    import oracle as orc
    zp = golden("zero_pose")
    zl = zp["vtrdyn_full_local_t"]
    g = golden("full_body_pos_precise")
    idx0 = np.arange(N0) % len(g["body"])
    body, lh, rh = (np.ascontiguousarray(g[k][idx0]) for k in ("body", "lh", "rh"))
    rng = np.random.default_rng(4747)
    Zt, Zl, Zr = zl[list(TORSO_Z)], zl[list(LEFT_Z)], zl[list(RIGHT_Z)]
    for i in range(N0):
        fam = FAMILIES[_family_of(i)]
        which = (i // 64 // NF) % 3 if i < 64 * 4 * NF else (i // NF) % 3    # 0 torso, 1 wrists, 2 all three fits
        v = i // NF if i >= 64 * 4 * NF else i
        hostile = (lambda M: _make_hostile(M, i, rng)) if fam == "hostile" else (lambda M: M)
        if which in (0, 2):
            body[i, 10] = 0.0
            body[i, TORSO_JOINTS, :] = hostile(_family_points(fam, Zt, v, rng))
        if which in (1, 2):
            for h, Zh in ((lh, Zl), (rh, Zr)):
                h[i, 0] = 0.0
                h[i, WRIST_JOINTS, :] = hostile(_family_points(fam, Zh, v, rng))
    odof, olr, obr = orc.full_body_pos(zl, zp["vtrdyn_full_global_t"], body, lh, rh, True)
    idx = np.arange(LATENCY_MAX_B + 1) % N0
    return dict(ins=(body[idx], lh[idx], rh[idx]), ref=(odof[idx], olr[idx], obr[idx]),
                status=orc.frame_status(odof)[idx], n0=(body, lh, rh))


def test_oracle_runs_the_families_without_surprises(kabsch_sets, fit_frames):
    """On the CPU: the oracle returns a unit quaternion for every fit whose points are finite (rank-deficient,
    rescaled and denormal ones included) and NaN for the others; the solver's oracle raises (status) on every NaN
    frame and on no finite one, and its DOFs are finite for every finite frame."""
    for npts, (Z, M, q) in kabsch_sets.items():
        fam = np.array([_family_of(i) for i in range(len(M))])
        finite_in = np.isfinite(M).all(axis=(1, 2))
        assert finite_in[fam != FAMILIES.index("hostile")].all()
        ok = np.isfinite(q).all(axis=1)
        assert ok[finite_in & (fam != FAMILIES.index("hostile"))].all(), npts
        assert not ok[~finite_in].any(), npts
        nrm = np.linalg.norm(q[ok].astype(np.float64), axis=1)
        assert np.abs(nrm - 1.0).max() < 1e-5, npts
    st, odof = fit_frames["status"][:N0], fit_frames["ref"][0][:N0]
    body, lh, rh = fit_frames["n0"]
    pts = np.concatenate([a.reshape(N0, -1) for a in (body, lh, rh)], axis=1)
    nan_in, finite_in = np.isnan(pts).any(axis=1), np.isfinite(pts).all(axis=1)
    assert nan_in.sum() >= 4 and (~finite_in & ~nan_in).sum() >= 4              # NaN and inf frames are there
    assert (st[nan_in] != 0).all() and (st[finite_in] == 0).all()               # raised: NaN always, finite never
    assert np.isfinite(odof[finite_in]).all()                                    # every scale, rank and zero pattern
    assert {(w, f) for w in range(3) for f in range(NF)} == {((i // 64 // NF) % 3, _family_of(i)) for i in range(64 * 4 * NF)}


@pytest.mark.gpu
@pytest.mark.parametrize("npts", [3, 5])
def test_cal_joint_quat_straddling_the_window_vs_oracle(gpu, kabsch_sets, npts):
    from rtg import ops
    Z, M, o = kabsch_sets[npts]
    for n in (len(Z), 65, 1):   # whole waves with a ragged tail, one wave and a lane, a single fit
        g = ops.cal_joint_quat(Z[:n], M[:n]).cpu().numpy()
        bad = np.nonzero((_bits(g) != _bits(o[:n])).any(axis=1))[0]
        assert bad.size == 0, (npts, n, bad.size, bad[:8], [FAMILIES[_family_of(int(i))] for i in bad[:8]])


def _solver():
    from rtg import _lib, assets
    from rtg.runtime import Solver
    zp = golden("zero_pose")
    return Solver(_lib.SOLVER_FULL_BODY_POS, zp["vtrdyn_full_local_t"], zp["vtrdyn_full_global_t"],
                  assets.parents("vtrdyn_full"), True)


def _check(S, fr, layout, sl, tag):
    from rtg.runtime import frame_status
    dev = [torch.from_numpy(np.ascontiguousarray(a[sl])).cuda() for a in fr["ins"]]
    if layout == "soa":
        dev = [t.permute(1, 2, 0).contiguous() for t in dev]
    dof, lr, br = S.retarget(dev, want_local_rot=True, want_body_rot=True, layout=layout)
    np.testing.assert_array_equal(frame_status(dof).cpu().numpy(), fr["status"][sl], err_msg=f"{tag}: status")
    for name, got, ref in (("dof", dof, fr["ref"][0]), ("local_rot", lr, fr["ref"][1]), ("body_rot", br, fr["ref"][2])):
        bad = np.nonzero((_bits(got.cpu().numpy()) != _bits(ref[sl])).reshape(len(ref[sl]), -1).any(axis=1))[0]
        assert bad.size == 0, (tag, name, bad.size, bad[:8], [FAMILIES[_family_of(int(i) % N0)] for i in bad[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("B", BATCHES)
def test_fits_straddling_the_window_vs_oracle(gpu, fit_frames, layout, B):
    """k_fbp_quad (8 and 16 frames per block), k_fbp_latency5 and k_solve_sides, with ragged last tiles."""
    from rtg import _lib
    assert _lib.build_info()["knobs"]["RTG_LATENCY_MAX_B"] == LATENCY_MAX_B
    _check(_solver(), fit_frames, layout, slice(0, B), f"B={B} {layout}")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_fits_straddling_the_window_single_frame_vs_oracle(gpu, fit_frames, layout):
    """B = 1 (k_fbp_frame1): frames of every whole-wave (fit, family) pair, lanes 0 and 63 of the hostile waves, and a
    stretch of the mixed tail."""
    S = _solver()
    frames = [64 * w + 5 for w in range(4 * NF)] + [64 * w + l for w in range(4 * NF) if w % NF == NF - 1 for l in (0, 63)]
    frames += list(range(64 * 4 * NF, 64 * 4 * NF + 4 * NF))
    for i in frames:
        _check(S, fit_frames, layout, slice(i, i + 1), f"frame {i} {layout}")

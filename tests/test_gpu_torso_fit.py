"""The Kabsch fits of the FULL_BODY_POS solver on adversarial point sets, through every kernel route and both input
layouts, bit for bit against the oracle (the general restatement of sgesdd): DOFs, local rotations, body rotations
(row 10 is the torso quaternion itself) and the per-frame status.  NaNs compare as NaN
(test_gpu_parity.py::test_quad_tile_ragged_batches_vs_oracle's rule).

The torso fit's zero-pose vectors have x = 0, so its A has a zero column and the fit runs a fixed path through the
SVD's rare-case branches; the point families below drive that path and every way out of it (rank-deficient sets,
zero planes, rescaled magnitudes, signed zeros, denormals, inf, NaN), in whole 64-frame waves of one family and
mixed within a wave, since the kernels' rare-case branches are decided per wave."""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

FAMILIES = ["rotation", "coplanar", "collinear", "mirrored", "zero", "duplicated", "tiny", "large", "signed_zero",
            "zero_plane", "inf", "nan"]
NF = len(FAMILIES)
HEAD = 128                      # frames [0, HEAD): families mixed within the waves
WAVES = 2 * NF                  # then one whole 64-frame wave per (torso | wrists, family)
SIDE_B = 49152 + 65             # smallest ragged side-kernel batch: a second tile with one live lane
N0 = 8255                       # distinct frames (the largest small-batch size); a longer batch repeats them
BATCHES = (17, 4089, 4097, 8255, SIDE_B)   # quad, quad, latency5, latency5 (ragged), side kernel; B = 1 apart
TORSO_JOINTS, WRIST_JOINTS = (17, 13, 11), (2, 6, 10, 14, 17)


def _bits(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def _rand_rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _family_points(fam, Z, rng):
    """An (n, 3) float32 point set M (relative to the fit's origin joint, which is put at 0 so M is exact) of the
    family for the zero vectors Z (n, 3)."""
    n = len(Z)
    good = Z.astype(np.float64) @ _rand_rot(rng).T + rng.normal(0.0, 1e-3, (n, 3))
    if fam == "rotation":
        M = good
    elif fam == "coplanar":
        a, b = rng.normal(size=3), rng.normal(size=3)
        c = rng.normal(size=(n, 2))
        M = 0.1 * (c[:, :1] * a + c[:, 1:] * b)
    elif fam == "collinear":
        M = 0.1 * rng.normal(size=(n, 1)) * rng.normal(size=3)
    elif fam == "mirrored":
        M = good * np.array([-1.0, 1.0, 1.0])
    elif fam == "zero":
        M = np.zeros((n, 3))
    elif fam == "duplicated":
        M = good.copy()
        M[1:1 + rng.integers(1, n)] = M[0]          # two or more (up to all) points equal
    elif fam == "tiny":
        M = good * 1e-12                            # below sgesdd's rescale threshold
    elif fam == "large":
        M = good * 1e3
    elif fam == "signed_zero":
        M = good.copy()
        M[rng.integers(n), rng.integers(3)] = rng.choice([0.0, -0.0, 1e-40, -1e-40, 1.4e-45])
    elif fam == "zero_plane":
        M = good.copy()
        M[:, rng.integers(3)] = rng.choice([0.0, -0.0])
    elif fam == "inf":
        M = good.copy()
        M[rng.integers(n), rng.integers(3)] = rng.choice([np.inf, -np.inf])
    elif fam == "nan":
        M = good.copy()
        M[rng.integers(n), rng.integers(3)] = np.nan
    else:
        raise KeyError(fam)
    return M.astype(np.float32)


def _plan(i):
    """(which, family) of frame i: which = 0 torso points, 1 both wrists' points, 2 all three fits."""
    if HEAD <= i < HEAD + 64 * WAVES:
        w = (i - HEAD) // 64
        return (0 if w < NF else 1), w % NF
    return i % 3, (i // 3) % NF


@pytest.fixture(scope="module")
def adversarial(gpu):
    """N0 synthetic frames with the fits' points overwritten, repeated up to SIDE_B, and the oracle's result for them
    (computed once on the N0; every frame is independent of its batch, so a shorter batch is a prefix)."""
    import oracle as orc
    from rtg import assets, ops
    from rtg.runtime import Topology
    zp = golden("zero_pose")
    zl = zp["vtrdyn_full_local_t"]
    T = Topology(assets.parents("vtrdyn_full"), assets.local_translation("vtrdyn_full"), assets.tree_quat("vtrdyn_full"))
    body, lh, rh = (t.cpu().numpy() for t in ops.synth_full_body(T, N0, seed=77))
    rng = np.random.default_rng(2025)
    Zt = zl[[11, 36, 34]]
    # the wrist fits' zero vectors are not needed exactly: any well-spread 5-point set gives the families their shape
    Zw = rng.normal(0.0, 0.05, (5, 3)).astype(np.float32)
    for i in range(N0):
        which, k = _plan(i)
        fam = FAMILIES[k]
        if which in (0, 2):
            body[i, 10] = 0.0
            body[i, TORSO_JOINTS, :] = _family_points(fam, Zt, rng)
        if which in (1, 2):
            # a NaN torso already raises the frame; give such frames ordinary wrists so the wrist families are not
            # all hidden behind it
            wf = "rotation" if (which == 2 and fam == "nan") else fam
            for h in (lh, rh):
                h[i, 0] = 0.0
                h[i, WRIST_JOINTS, :] = _family_points(wf, Zw, rng)
    odof, olr, obr = orc.full_body_pos(zl, zp["vtrdyn_full_global_t"], body, lh, rh, True)
    idx = np.arange(SIDE_B) % N0
    return dict(ins=(body[idx], lh[idx], rh[idx]), ref=(odof[idx], olr[idx], obr[idx]),
                status=orc.frame_status(odof)[idx])


def _solver(zl=None):
    from rtg import _lib, assets
    from rtg.runtime import Solver
    zp = golden("zero_pose")
    return Solver(_lib.SOLVER_FULL_BODY_POS, zp["vtrdyn_full_local_t"] if zl is None else zl,
                  zp["vtrdyn_full_global_t"], assets.parents("vtrdyn_full"), True)


def _run(S, ins, layout, sl):
    dev = [torch.from_numpy(np.ascontiguousarray(a[sl])).cuda() for a in ins]
    if layout == "soa":
        dev = [t.permute(1, 2, 0).contiguous() for t in dev]
    dof, lr, br = S.retarget(dev, want_local_rot=True, want_body_rot=True, layout=layout)
    return dof, lr.cpu().numpy(), br.cpu().numpy()


def _check(S, ins, ref, status, layout, sl, tag):
    from rtg.runtime import frame_status
    dof, lr, br = _run(S, ins, layout, sl)
    np.testing.assert_array_equal(frame_status(dof).cpu().numpy(), status[sl], err_msg=f"{tag}: status")
    np.testing.assert_array_equal(_bits(dof.cpu().numpy()), _bits(ref[0][sl]), err_msg=f"{tag}: dof")
    np.testing.assert_array_equal(_bits(lr), _bits(ref[1][sl]), err_msg=f"{tag}: local_rot")
    np.testing.assert_array_equal(_bits(br), _bits(ref[2][sl]), err_msg=f"{tag}: body_rot")


def test_families_behave_as_the_reference_does(adversarial):
    """The plan covers every (fit, family) pair in whole waves and mixed; a NaN point makes the frame raise (status 1),
    an inf point gives NaN outputs or (where a product with a zero of the zero pose makes a NaN in A) raises too."""
    st, odof = adversarial["status"], adversarial["ref"][0]
    seen = {(_plan(i)) for i in range(HEAD)} | {(_plan(i)) for i in range(HEAD + 64 * WAVES, 4089)}
    assert seen == {(w, k) for w in range(3) for k in range(NF)}
    for i in range(4089):
        which, k = _plan(i)
        if FAMILIES[k] == "nan":
            assert st[i] == 1, i
        elif FAMILIES[k] == "inf":
            assert np.isnan(odof[i]).any(), i
    assert (st[:HEAD + 64 * WAVES] == 0).any()


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("B", BATCHES)
def test_adversarial_fits_vs_oracle(adversarial, layout, B):
    """Each batched kernel route (k_fbp_quad, k_fbp_latency5, k_solve_sides) on the adversarial frames."""
    _check(_solver(), adversarial["ins"], adversarial["ref"], adversarial["status"], layout, slice(0, B), f"B={B}")


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_adversarial_fits_single_frame_vs_oracle(adversarial, layout):
    """B = 1 (k_fbp_frame1): one launch per (fit, family) pair of the mixed head, and one frame of each whole wave."""
    S = _solver()
    frames = list(range(3 * NF)) + [HEAD + 64 * w + 5 for w in range(WAVES)]
    for i in frames:
        _check(S, adversarial["ins"], adversarial["ref"], adversarial["status"], layout, slice(i, i + 1), f"frame {i}")


def _zero_pose_variant(name):
    zl = golden("zero_pose")["vtrdyn_full_local_t"].copy()
    rows = {"one_nonzero_x": [36], "all_nonzero_x": [11, 36, 34], "negative_zero_x": [11, 36, 34]}[name]
    assert (zl[[11, 36, 34], 0] == 0).all()
    zl[rows, 0] = -0.0 if name == "negative_zero_x" else np.float32(0.0123)
    return zl


@pytest.mark.parametrize("name", ["one_nonzero_x", "all_nonzero_x", "negative_zero_x"])
def test_zero_poses_off_the_zero_column(adversarial, name):
    """Zero poses whose torso vectors do not have x = +0: a nonzero x on one or on all of rows 11 / 36 / 34 (the
    torso A has no zero column) and -0.0 there (column 0 of A is still +-0, with the other sign).  The oracle takes
    the same zero pose; the side kernel (B = 49152 + 65) and k_fbp_quad (B = 17), both layouts."""
    import oracle as orc
    zp = golden("zero_pose")
    zl = _zero_pose_variant(name)
    n = 64 * 40 + 65   # oracle frames: the head, every whole torso wave, part of the wrist waves; the tail reuses them
    ins = tuple(a[:n] for a in adversarial["ins"])
    odof, olr, obr = orc.full_body_pos(zl, zp["vtrdyn_full_global_t"], *ins, True)
    S = _solver(zl)
    idx = np.arange(SIDE_B) % n
    big = tuple(a[idx] for a in ins)
    ref = (odof[idx], olr[idx], obr[idx])
    status = orc.frame_status(odof)[idx]
    for layout in ("aos", "soa"):
        _check(S, big, ref, status, layout, slice(0, SIDE_B), f"{name} {layout} B={SIDE_B}")
        _check(S, big, ref, status, layout, slice(0, 17), f"{name} {layout} B=17")


def test_goldens_unchanged_through_the_side_kernel(gpu):
    """full_body_pos_precise tiled to a ragged B > 49152 batch (the side kernel) equals its small-batch result and
    the oracle, bit for bit."""
    import oracle as orc
    zp = golden("zero_pose")
    d = golden("full_body_pos_precise")
    ins = tuple(np.ascontiguousarray(d[k]) for k in ("body", "lh", "rh"))
    n = len(ins[0])
    S = _solver()
    dof_s, lr_s, br_s = _run(S, ins, "aos", slice(0, n))
    odof, olr, obr = orc.full_body_pos(zp["vtrdyn_full_local_t"], zp["vtrdyn_full_global_t"], *ins, True)
    np.testing.assert_array_equal(_bits(dof_s.cpu().numpy()), _bits(odof))
    np.testing.assert_array_equal(_bits(lr_s), _bits(olr))
    np.testing.assert_array_equal(_bits(br_s), _bits(obr))
    idx = np.arange(SIDE_B) % n
    big = tuple(a[idx] for a in ins)
    for layout in ("aos", "soa"):
        dof_b, lr_b, br_b = _run(S, big, layout, slice(0, SIDE_B))
        np.testing.assert_array_equal(_bits(dof_b.cpu().numpy()), _bits(odof[idx]), err_msg=layout)
        np.testing.assert_array_equal(_bits(lr_b), _bits(olr[idx]), err_msg=layout)
        np.testing.assert_array_equal(_bits(br_b), _bits(obr[idx]), err_msg=layout)

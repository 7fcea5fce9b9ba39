"""The hostile batches of tests/motion_prep_frames.py on the host: the C oracle's rescale_motion, quat_between and
rebuild_vtrdyn against the reference's own outputs for them (tests/golden/motion_prep_adversarial.npz, recorded by
tools/make_golden.py), the branches the batches promise, and the ingest flag's predicate against np.allclose -- the
conditions tests/test_gpu_motion_prep_hostile.py rests on.

Rescale, quat_between and every rebuilt row but 0 and 10: bit for bit, NaN-aware (retarget_to_ref.bits).  Rows 0 and 10
are Kabsch fits, whose finite values carry the reference's VML square-root ulp: the same NaN / finite pattern in every
family, and on the tame family the 6e-8 that tests/test_gpu_dropin.py::test_main_retarget_from_global_translation
allows.  (The hostile fits' values are held to the reference by tests/test_other_solvers_host.py and to the oracle by
tests/test_gpu_fit_division.py.)"""
import zlib

import numpy as np
import pytest

from conftest import golden

import motion_prep_frames as mp
import oracle as orc
from retarget_to_ref import bits

IDENT = np.float32([0, 0, 0, 1])
DIR = [-1.0, -1.0, 1.0]
OTHER_ROWS = [r for r in range(21) if r not in (0, 10)]


def _tree():
    from rtg import assets
    return assets.parents("vtrdyn"), golden("zero_pose")["vtrdyn_local_t"]


def _is_identity(q):
    return bool((bits(q) == bits(IDENT)).all())


def test_the_fixture_was_recorded_from_these_inputs():
    g = golden("motion_prep_adversarial")
    from rtg import assets
    zp = golden("zero_pose")
    crc = 0
    for v1, v2 in mp.fixture_pairs().values():
        crc = zlib.crc32(v1.tobytes() + v2.tobytes(), crc)
    for fam in mp.MOTION_FAMILIES:
        crc = zlib.crc32(mp.fixture_motion(fam).tobytes(), crc)
    trees = mp.topologies({n: assets.parents(n) for n in ("vtrdyn", "vtrdyn_full")},
                          {n: zp[f"{n}_local_t"] for n in ("vtrdyn", "vtrdyn_full")})
    for par, lt, m in trees.values():
        crc = zlib.crc32(par.tobytes() + lt.tobytes() + m.tobytes(), crc)
    assert crc == int(g["input_crc"]), "the helper's arrays moved: record again"
    assert g["families"].tolist() == list(mp.MOTION_FAMILIES) and g["pairs"].tolist() == list(mp.fixture_pairs())
    # deterministic, and a *_single family touches one element class per touched frame
    np.testing.assert_array_equal(bits(mp.motions("nan_single", 513)), bits(mp.motions("nan_single", 513)))
    assert mp.single_frames(513) == [0, 1, 63, 64, 127, 128, 191, 192, 255, 256, 319, 320, 383, 384, 447, 448, 511, 512]
    assert {mp.single_joint(i) for i in range(11)} >= {0, 10, 1, 4, 5, 14, 3, 6}
    bad = np.isnan(mp.motions("nan_single", 513)).any(axis=(1, 2))
    assert np.flatnonzero(bad).tolist() == mp.single_frames(513)


def test_quat_between_matches_the_recorded_reference():
    """Every pair batch: the oracle equals the reference's bits, and the batch takes the branch its name says -- the
    identity for a largest norm of 0, 1e-45 (norm 0), 1e-6f - ulp and 1e-6f, on either side; not for 1e-6f + ulp, 1e-5,
    one NaN row or one inf row among small ones."""
    g = golden("motion_prep_adversarial")
    pairs = mp.fixture_pairs()
    for name, (v1, v2) in pairs.items():
        with np.errstate(all="ignore"):
            q = orc.quat_between(v1, v2)
        np.testing.assert_array_equal(bits(q), bits(g[f"qb_{name}"]), err_msg=name)
        assert _is_identity(q) == mp.pair_identity(name), name
        if not mp.pair_identity(name):
            assert not (bits(q) == bits(IDENT)).all(axis=1).any() or name == "mixed", name
        print(f"quat_between {name}: {len(q)} rows bit-equal to the reference, identity branch {_is_identity(q)}, "
              f"{int(np.isnan(q).any(axis=1).sum())} NaN rows")
    for side in (1, 2):                      # the deciding rows are what they say
        for name, (length, rest, _) in mp.DECISIONS.items():
            v = pairs[f"v{side}_{name}"][side - 1]
            n = np.sqrt(((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]))
            want = np.float32(0) if name == "1e-45" else length
            assert n.max() == want and (n == n.max()).sum() == (1 if want else len(n)), (side, name)
    # the mixed batch reaches what it is for: a zero real part, a squared norm that underflows, one that overflows
    v1, v2, at = mp.mixed_rows(24)
    q = g["qb_mixed"]
    assert np.isnan(q[at["zero_v1"]]).all() and np.isnan(q[at["zero_v2"]]).all() and np.isnan(q[at["scale_1e-30"]]).all()
    assert q[at["antiparallel"]][3] == 0                   # 1 + dot == 0 beside a cross product of rounding errors
    assert (v2[at["antiparallel_ulp"]] != -v1[at["antiparallel_ulp"]]).sum() == 1
    assert np.isfinite(q[at["scale_1e-19"]]).all() and np.isfinite(q[at["scale_1e18"]]).all()
    assert (bits(q[at["parallel_3x"]][3]) == bits(np.float32(1))).all()


def test_rescale_matches_the_recorded_reference():
    """rescale_motion with dir = [-1, -1, 1] and without, every family: the oracle equals the reference's bits; a scale_*
    family has every frame non-finite or none, as the helper states."""
    g = golden("motion_prep_adversarial")
    par, zl = _tree()
    for fam in mp.MOTION_FAMILIES:
        m = mp.fixture_motion(fam)
        with np.errstate(all="ignore"):
            r, rn = orc.rescale_motion(par, zl, m, dir=DIR), orc.rescale_motion(par, zl, m)
        np.testing.assert_array_equal(bits(r), bits(g[f"m_{fam}_rescaled"]), err_msg=fam)
        np.testing.assert_array_equal(bits(rn), bits(g[f"m_{fam}_rescaled_nodir"]), err_msg=fam)
        bad = ~np.isfinite(r).all(axis=(1, 2))
        np.testing.assert_array_equal(bad, ~np.isfinite(rn).all(axis=(1, 2)))
        print(f"rescale {fam}: {len(m)} frames bit-equal to the reference, {int(bad.sum())} of {len(m)} non-finite")
        if fam.startswith("scale_"):
            assert bad.all() if mp.SCALE_NONFINITE[float(fam[6:])] else not bad.any(), fam
        if fam in mp.SINGLES[:4]:
            assert np.flatnonzero(bad).tolist() == mp.single_frames(len(m)), fam
        if fam in ("tame", "huge_single", "coplanar_torso", "mirrored"):
            assert not bad.any(), fam


def test_rescale_on_other_trees_matches_the_recorded_reference():
    """The 21- and 59-joint zero poses, a one-joint tree and a 5-chain whose local_t rows are zero, 1e-30, 1e25 and NaN
    long (the scale's divisor 0, 0 after underflow, inf, NaN)."""
    from rtg import assets
    g = golden("motion_prep_adversarial")
    zp = golden("zero_pose")
    trees = mp.topologies({n: assets.parents(n) for n in ("vtrdyn", "vtrdyn_full")},
                          {n: zp[f"{n}_local_t"] for n in ("vtrdyn", "vtrdyn_full")})
    assert list(trees) == ["vtrdyn", "vtrdyn_full", "one", "chain5"]
    for name, (par, lt, m) in trees.items():
        with np.errstate(all="ignore"):
            r = orc.rescale_motion(par, lt, m)
        np.testing.assert_array_equal(bits(r), bits(g[f"topo_{name}_rescaled"]), err_msg=name)
    r = g["topo_chain5_rescaled"]
    # |zl| = 0 (twice: the 1e-30 row's square underflows): scale inf, the joint on its parent; |zl| = inf: scale 0,
    # d / 0 = +-inf; |zl| = NaN: NaN, on a parent that is already non-finite
    assert (r[:, 1] == r[:, 0]).all() and (r[:, 2] == r[:, 1]).all()
    assert np.isinf(r[:, 3]).all() and np.isnan(r[:, 4]).all()


def _kabsch_nan(m, zl):
    """(B, 2) bool: the fit of joint 0 / joint 10 of a frame has a NaN in its matrix."""
    with np.errstate(all="ignore"):
        A = [np.einsum("bji,jk->bik", m[:, pts] - m[:, [c]], zl[pts]) for c, pts in ((0, [4, 1, 7]), (10, [17, 13, 11]))]
    return np.isnan(np.stack(A, axis=1)).any(axis=(2, 3))


def test_rebuild_matches_the_recorded_reference():
    """rebuild_vtrdyn on the reference's rescaled motion and on the raw motion of every family.  Rows other than 0 and
    10: the oracle's bits equal the reference's, the batches whose SVD raised included (recorded there through the
    per-bone calls).  Rows 0 and 10: NaN where the reference has NaN and finite where it is finite; where the batch
    raised, NaN in every frame whose Kabsch matrix holds one; on the tame family within 6e-8."""
    g = golden("motion_prep_adversarial")
    par, zl = _tree()
    raised = []
    for fam in mp.MOTION_FAMILIES:
        for key, x in ((f"m_{fam}_rebuild", g[f"m_{fam}_rescaled"]), (f"m_{fam}_rebuild_raw", mp.fixture_motion(fam))):
            with np.errstate(all="ignore"):
                gr, rt = orc.rebuild_vtrdyn(par, zl, x)
            ref = g[key]
            np.testing.assert_array_equal(bits(rt), bits(x[:, 0]), err_msg=key)
            np.testing.assert_array_equal(bits(gr[:, OTHER_ROWS]), bits(ref[:, OTHER_ROWS]), err_msg=key)
            k = gr[:, [0, 10]]
            if int(g[f"{key}_status"]):
                raised.append(key)
                assert "linalg.svd" in str(g[f"{key}_message"])
                nan = _kabsch_nan(x, zl)
                assert nan.any() and np.isnan(k[nan]).all(), key
                assert mp.svd_input_has_nan(x, zl)
            else:
                assert not mp.svd_input_has_nan(x, zl), key
                np.testing.assert_array_equal(np.isnan(k), np.isnan(ref[:, [0, 10]]), err_msg=key)
                np.testing.assert_array_equal(np.isfinite(k), np.isfinite(ref[:, [0, 10]]), err_msg=key)
            if fam == "tame":
                assert not int(g[f"{key}_status"])
                assert np.abs(k.astype(np.float64) - ref[:, [0, 10]]).max() <= 6e-8, key
            nanf = np.isnan(gr).any(axis=(1, 2))
            print(f"rebuild {key[2:]}: {len(x)} frames, rows other than 0 / 10 bit-equal to the reference, "
                  f"{int(nanf.sum())} of {len(x)} frames with a NaN row, the reference's SVD "
                  f"{'raised' if int(g[f'{key}_status']) else 'returned'}")
    # only a NaN that reaches joints 0, 1, 4, 7, 10, 11, 13 or 17 raises: the families that cannot put one there return
    for fam in ("tame", "scale_1e-20", "scale_1e-18", "scale_1e15", "scale_1e19", "scale_1e25", "scale_1e37",
                "coplanar_torso", "mirrored") + tuple(f"tiny_bone_every_frame_{d}" for d in ("eps_below", "eps", "eps_above", "1e-5")):
        assert f"m_{fam}_rebuild" not in raised and f"m_{fam}_rebuild_raw" not in raised, fam
    assert "m_nan_single_rebuild_raw" in raised and "m_inf_single_rebuild_raw" in raised
    assert "m_zero_bone_every_frame_15_rebuild_raw" not in raised and "m_collapsed_rebuild_raw" not in raised


def test_rebuild_takes_the_batch_branch_where_the_family_says():
    """On the oracle's own output, raw motions: tiny_bone_every_frame_<d> turns row 14 (the parent of bone 15) to the
    identity for d = 0, 1e-45, 1e-6f - ulp and 1e-6f and not for 1e-6f + ulp and 1e-5; zero_bone_every_frame_<j> turns
    the row of j's parent; a single zero bone turns no row; collapsed turns every row it can."""
    par, zl = _tree()
    for B in (16, 513):
        with np.errstate(all="ignore"):
            tame, _ = orc.rebuild_vtrdyn(par, zl, mp.motions("tame", B))
            ident_rows = lambda g: [r for r in OTHER_ROWS if _is_identity(g[:, r])]   # noqa: E731
            base = ident_rows(tame)
            assert base == list(mp.LEAF_JOINTS)          # a leaf has no child: its row stays the identity
            for d, (_, _, ident) in mp.DECISIONS.items():
                gr, _ = orc.rebuild_vtrdyn(par, zl, mp.motions(f"tiny_bone_every_frame_{d}", B))
                assert ident_rows(gr) == sorted(base + [14] * ident), (d, B)
            for j in mp.ZERO_BONE_JOINTS:
                gr, _ = orc.rebuild_vtrdyn(par, zl, mp.motions(f"zero_bone_every_frame_{j}", B))
                assert ident_rows(gr) == sorted(base + [int(par[j])]), (j, B)
            gr, _ = orc.rebuild_vtrdyn(par, zl, mp.motions("zero_bone_single", B))
            assert ident_rows(gr) == base
            gr, _ = orc.rebuild_vtrdyn(par, zl, mp.motions("collapsed", B))
            assert ident_rows(gr) == OTHER_ROWS
            for row in (0, B - 1):                       # a NaN or inf frame in a degenerate batch: no identity
                for v in (np.nan, np.inf):
                    gr, _ = orc.rebuild_vtrdyn(par, zl, mp.rebuild_decision(B, mp.TINY_BONE, v, row, 1e-7))
                    assert ident_rows(gr) == base, (row, v, B)


@pytest.mark.parametrize("k", [0, 12, 14, 24, 26, 68])
def test_ingest_predicate_is_allclose(k):
    """not np.allclose(frame, 0) equals !(|x| <= 1e-8f) over the frame's 69 floats, for every boundary value at position
    k (12 .. 14 and 24 .. 26 are joints 4 and 8, which the 23 -> 21 map drops)."""
    for v in mp.ingest_values():
        frame = np.zeros(69, np.float32)
        frame[k] = v
        assert (not np.allclose(frame, 0)) == mp.carries_data(frame), v
    up = np.nextafter(mp.ATOL, np.float32(1))
    down = np.nextafter(mp.ATOL, np.float32(0))
    for v, carries in ((0.0, False), (-0.0, False), (1e-45, False), (down, False), (mp.ATOL, False), (-mp.ATOL, False),
                       (up, True), (-up, True), (1e-7, True), (np.nan, True), (np.inf, True), (-np.inf, True)):
        frame = np.zeros(69, np.float32)
        frame[k] = v
        assert mp.carries_data(frame) == carries and (not np.allclose(frame, 0)) == carries, v

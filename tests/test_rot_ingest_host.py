"""The zero-pose transform of mocap rotations, host side (no GPU): the oracle composition the GPU tests compare against
equals the reference's recorded outputs bit for bit, the constants rebuild from the committed assets, and the library's
argument checks answer before any HIP call."""
import ctypes

import numpy as np
import pytest

import rot_ingest_frames as rf
from conftest import golden
from rot_ingest_frames import bits, compose, conj


@pytest.fixture(scope="module")
def fx():
    return golden("zero_pose_transform")


def _forms(fx):
    """(fixture output key, input key, src, pre, post) of every recorded reference output."""
    p21, p59 = conj(fx["t2zero_vtrdyn"]), conj(fx["t2zero_vtrdyn_full"])
    out = []
    for tag in ("unit_21", "family_21"):
        out.append((f"out_{tag}_vtrdyn", tag, None, fx["pre_vtrdyn"], p21))
        out.append((f"out_{tag}_broadcast", tag, None, fx["pre_broadcast"], p21))
    for tag in ("unit_59", "family_59"):
        out.append((f"out_{tag}_vtrdyn_full", tag, None, fx["pre_vtrdyn_full"], p59))
    out.append(("out_broadcast_23_vtrdyn", "broadcast_23", rf.BODY23_TO_21, fx["pre_vtrdyn"], p21))
    out.append(("out_broadcast_23_broadcast", "broadcast_23", rf.BODY23_TO_21, fx["pre_broadcast"], p21))
    out.append(("out_broadcast_23_full_scatter", "broadcast_23", rf.BODY23_TO_21, fx["pre_vtrdyn_full"],
                p59[rf.BODY21_IN_FULL59]))
    return out


def test_fixture_inputs_are_the_helper_frames(fx):
    """The recorded inputs equal freshly built ones: the GPU tests' frames are the frames the reference saw."""
    assert str(fx["meta_source"].reshape(-1)[0]) in ("retarget.utils.parse_mocap", "primitives")
    assert [str(n) for n in fx["family_names"]] == rf.FAMILY_NAMES and len(rf.FAMILY_NAMES) == 18
    for key, fresh in (("unit_21", rf.unit_frames(64, 21)), ("unit_59", rf.unit_frames(64, 59)),
                       ("family_21", rf.family_frames(21)), ("family_59", rf.family_frames(59)),
                       ("broadcast_23", rf.broadcast_frames(64))):
        assert fx[key].dtype == np.float32 and fx[key].shape == fresh.shape, key
        assert np.array_equal(bits(fx[key]), bits(fresh)), key
    fam = fx["family_21"].reshape(18, rf.PER_FAMILY, 21, 4)
    k = rf.FAMILY_NAMES.index
    assert np.isnan(fam[k("nan")]).any(axis=(1, 2)).all() and np.isinf(fam[k("inf")]).any(axis=(1, 2)).all()
    assert (np.abs(fam[k("zero_row")]).sum(axis=-1) == 0).any(axis=1).all()


def test_oracle_composition_equals_every_reference_output(fx):
    """orc.quat_mul_norm twice, with the fixture's constants, against all recorded outputs: every family bit for bit,
    NaN compared as NaN, the sign of zero compared."""
    for okey, ikey, src, pre, post in _forms(fx):
        got = compose(fx[ikey], src, pre, post)
        want = fx[okey]
        assert got.shape == want.shape, okey
        bad = np.argwhere(bits(got) != bits(want))
        assert not len(bad), (okey, len(bad), bad[:4].tolist())


def test_constants_rebuild_from_the_committed_assets(fx):
    """t2zero from oracle FK over assets/vtrdyn.npz / vtrdyn_full.npz (the zero-pose trees: the reference uses its
    t-pose trees, which differ in translations only) and the axis rotations from the oracle's quat_from_angle_axis
    equal the reference's recorded constants bit for bit."""
    for asset in ("vtrdyn", "vtrdyn_full"):
        got = rf.t2zero_from_assets(asset)
        assert np.array_equal(bits(got), bits(fx[f"t2zero_{asset}"])), asset
    assert np.array_equal(bits(rf.axis_quat(rf.HALF_PI, 2)), bits(fx["pre_vtrdyn"]))
    assert np.array_equal(bits(rf.axis_quat(rf.HALF_PI, 2)), bits(fx["pre_vtrdyn_full"]))
    assert np.array_equal(bits(rf.axis_quat(rf.HALF_PI, 0)), bits(fx["pre_broadcast"]))
    # the four turned joints make t2zero more than a table of identities
    assert (np.abs(fx["t2zero_vtrdyn"][:, 3]) < 0.99).sum() >= 4


def test_python_side_without_a_gpu():
    """Nothing runs at import or in a constructor; the tile constants repeat the library's; shapes are checked."""
    from rtg import _lib, ingest
    info = _lib.build_info()
    assert ingest.ROT_TILE_AOS == info["knobs"]["RTG_ROT_INGEST_TILE_AOS"]
    assert ingest.ROT_TILE_SOA == info["knobs"]["RTG_ROT_INGEST_TILE_SOA"]
    assert ingest.BODY23_TO_21 == rf.BODY23_TO_21 and ingest.BODY21_IN_FULL59 == rf.BODY21_IN_FULL59
    for name in ("vtrdyn", "vtrdyn_full", "vtrdyn_broadcast", "vtrdyn_full_from_broadcast"):
        t = getattr(ingest.ZeroPoseTransform, name)()
        assert t._build is not None and not t._handles        # constants and handle still to be built
    assert ingest.ZeroPoseTransform.vtrdyn_broadcast().J_in == 23
    g = ingest.ZeroPoseTransform(3, [2, 2, 0, 1], [0, 0, 0, 2], np.ones((4, 4)))
    assert (g.J_in, g.J_out) == (3, 4) and g.src.tolist() == [2, 2, 0, 1]
    with pytest.raises(ValueError):
        ingest.ZeroPoseTransform(3, [0, 1], [0, 0, 0, 1], np.ones((3, 4)))
    with pytest.raises(ValueError):
        ingest.ZeroPoseTransform(3, None, [0, 0, 1], np.ones((3, 4)))
    for fn in ("vtrdyn_zero_pose_transform", "vtrdyn_full_zero_pose_transform",
               "vtrdyn_broadcast_zero_pose_transform", "zero_pose_transform_quat", "ingest_rotations"):
        assert callable(getattr(ingest, fn)) and fn in ingest.__all__


def test_library_rejects_invalid_arguments_before_any_hip_call():
    """ABI 7, the three symbols, and RTG_ERR_INVALID_ARGUMENT with a message for every bad argument that can be told
    without a handle (a handle needs a device: the overlap check, which needs the handle's J, is a GPU test)."""
    from rtg import _lib
    lib = _lib.lib()
    assert lib.rtg_abi_version() == _lib.ABI_VERSION == 7
    for name in ("rtg_rot_ingest_create", "rtg_rot_ingest_destroy", "rtg_rot_ingest_f32"):
        assert hasattr(lib, name)
    INVALID = 1
    ip, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    pre = np.array([0, 0, 0, 1], np.float32)
    post = np.tile(pre, (64, 1))
    ident = np.arange(64, dtype=np.int32)

    def create(J_in, J_out, src, pre_, post_, out=True):
        h = ctypes.c_void_p()
        rc = lib.rtg_rot_ingest_create(J_in, J_out, None if src is None else src.ctypes.data_as(ip),
                                       None if pre_ is None else pre_.ctypes.data_as(fp),
                                       None if post_ is None else post_.ctypes.data_as(fp),
                                       ctypes.byref(h) if out else None)
        return rc, lib.rtg_last_error().decode(), h

    bad_src = ident.copy()
    bad_src[5] = 21
    neg_src = ident.copy()
    neg_src[0] = -1
    for args, word in (((0, 21, ident, pre, post), "outside 1..64"), ((21, 0, ident, pre, post), "outside 1..64"),
                       ((65, 21, ident, pre, post), "outside 1..64"), ((21, 65, ident, pre, post), "outside 1..64"),
                       ((21, 21, bad_src, pre, post), "src[5] = 21"), ((21, 21, neg_src, pre, post), "src[0] = -1"),
                       ((23, 21, None, pre, post), "identity"), ((21, 21, ident, None, post), "NULL"),
                       ((21, 21, ident, pre, None), "NULL")):
        rc, msg, h = create(*args)
        assert rc == INVALID and word in msg and "rtg_rot_ingest_create" in msg and not h.value, (args[:2], rc, msg)
    rc, msg, _ = create(21, 21, ident, pre, post, out=False)
    assert rc == INVALID and "out is NULL" in msg

    stream = ctypes.c_void_p()
    buf = np.zeros(64 * 4 + 8, np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    a, b = ctypes.c_void_p(base), ctypes.c_void_p(base + 512)

    def launch(h, q, B, layout, out):
        rc = lib.rtg_rot_ingest_f32(h, q, B, layout, out, stream)
        return rc, lib.rtg_last_error().decode()

    for args, word in (((None, a, -1, 0, b), "B < 0"), ((None, a, 4, 2, b), "bad layout 2"),
                       ((None, a, 4, -1, b), "bad layout -1"), ((None, None, 4, 0, b), "NULL buffer"),
                       ((None, a, 4, 1, None), "NULL buffer"),
                       ((None, ctypes.c_void_p(base + 4), 4, 0, b), "16-byte aligned"),
                       ((None, a, 4, 1, ctypes.c_void_p(base + 520)), "16-byte aligned"),
                       ((None, a, 4, 0, b), "NULL handle"), ((None, a, 0, 0, b), "NULL handle")):
        rc, msg = launch(*args)
        assert rc == INVALID and word in msg and "rtg_rot_ingest_f32" in msg, (rc, msg)
    lib.rtg_rot_ingest_destroy(None)   # a no-op

"""The zero-pose transform of mocap rotations on the GPU (rtg_rot_ingest_f32, rtg.ingest.ZeroPoseTransform): every
comparison is bit for bit (NaN as NaN, the sign of zero included) against the oracle composition of
tests/rot_ingest_frames.py, which tests/test_rot_ingest_host.py ties to the reference's recorded outputs.

"The four forms": 21 -> 21 (vtrdyn), 59 -> 59 (vtrdyn_full), 23 -> 21 with the broadcast constants, 23 -> 21 with the
59-joint constants.  T is the layout's tile size (frames per block)."""
import ctypes

import numpy as np
import pytest
import torch

import other_solver_frames as osf
import rot_ingest_frames as rf
from conftest import golden
from rot_ingest_frames import bits, compose, conj

pytestmark = pytest.mark.gpu

FORMS = ("vtrdyn", "vtrdyn_full", "vtrdyn_broadcast", "vtrdyn_full_from_broadcast")
LAYOUTS = ("aos", "soa")
BMAX = 4097


def _tile(layout):
    from rtg import ingest
    return ingest.ROT_TILE_SOA if layout == "soa" else ingest.ROT_TILE_AOS


@pytest.fixture(scope="module")
def fx():
    return golden("zero_pose_transform")


@pytest.fixture(scope="module")
def forms(gpu, fx):
    """name -> dict(tr: the ZeroPoseTransform, J_in, src, pre, post: the REFERENCE's recorded constants, q: BMAX
    ordinary (unit) frames, want: their oracle composition, computed once)."""
    from rtg import ingest
    p21, p59 = conj(fx["t2zero_vtrdyn"]), conj(fx["t2zero_vtrdyn_full"])
    consts = {"vtrdyn": (21, None, fx["pre_vtrdyn"], p21), "vtrdyn_full": (59, None, fx["pre_vtrdyn_full"], p59),
              "vtrdyn_broadcast": (23, rf.BODY23_TO_21, fx["pre_broadcast"], p21),
              "vtrdyn_full_from_broadcast": (23, rf.BODY23_TO_21, fx["pre_vtrdyn_full"], p59[rf.BODY21_IN_FULL59])}
    out = {}
    for k, name in enumerate(FORMS):
        J_in, src, pre, post = consts[name]
        q = rf.unit_frames(BMAX, J_in, seed=7400 + k)
        out[name] = dict(tr=getattr(ingest.ZeroPoseTransform, name)(), J_in=J_in, src=src, pre=pre, post=post, q=q,
                         want=compose(q, src, pre, post))
    return out


def run(tr, q, layout):
    """(B, J_in, 4) host frames -> (B, J_out, 4) host result of one launch in `layout`."""
    out = tr(torch.from_numpy(np.ascontiguousarray(q)), layout=layout)
    if layout == "soa":
        assert tuple(out.shape) == (tr.J_out, 4, len(q))
        out = out.permute(2, 0, 1)
    else:
        assert tuple(out.shape) == (len(q), tr.J_out, 4)
    return out.cpu().numpy()


def same(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert not len(bad), (what, len(bad), bad[:4].tolist())


def batch_sizes(layout):
    T = _tile(layout)
    return (1, T - 1, T, T + 1, 3 * T + 5, BMAX)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", FORMS)
def test_batch_sizes_and_determinism(forms, name, layout):
    f = forms[name]
    for B in batch_sizes(layout):
        got = run(f["tr"], f["q"][:B], layout)
        same(got, f["want"][:B], (name, layout, B))
    again = run(f["tr"], f["q"], layout)
    assert np.array_equal(bits(again), bits(got)), "two launches differ"


def hostile_row(fam, rng, v):
    """One quaternion row (float64) of family `fam` (the 18 of tests/other_solver_frames.py), variant v."""
    q = osf.rand_unit(rng)
    if fam == "unit":
        return q
    if fam == "nonunit":
        return q * rng.uniform(0.5, 2.0)
    if fam == "near_unit":   # |q|^2 k codes above 1.0f or 2 k below it: on the 33-code table, near its edges and off it
                             # (test_near_unit_table_edges lands on the edge codes themselves)
        return q * osf.near_unit_factor((0, 1, -1, 15, -15, 16, -16, 17, -17, 18, -18, 40, -40)[v % 13])
    if fam == "negated":
        return -q
    if fam == "identity":
        return np.array([0.0, 0.0, 0.0, 1.0])
    if fam == "relative_identity":
        return np.array([0.0, 0.0, 0.0, -1.0 if v % 2 else 1.0])
    if fam == "half_turn":
        return osf.axis_quat(v % 3, np.pi) if v % 4 != 3 else np.append(osf._unit3(rng), 0.0)
    if fam == "gimbal":
        return osf.gimbal_quat(("YXZ", "ZYX", "XYZ")[v % 3], rng, v)
    if fam == "w_table_edges":
        return osf.w_edge_quat(rng, v)
    if fam.startswith("scale_"):
        return q * float(fam[6:])
    if fam == "zero_row":
        return np.zeros(4)
    q[int(rng.integers(4))] = osf._special(fam, rng)   # nan, inf, signed_zero
    return q


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", FORMS)
def test_hostile_families(forms, fx, name, layout):
    """Every family once on all rows of a frame and once on one row only (13 variants each, the row moving), then the
    reference's own family frames for the form's input width."""
    f = forms[name]
    J = f["J_in"]
    rng = np.random.default_rng(7500 + J)
    frames = []
    for k, fam in enumerate(rf.FAMILY_NAMES):
        for v in range(13):
            frames.append(np.stack([hostile_row(fam, rng, v + r) for r in range(J)]))
            one = f["q"][len(frames)].astype(np.float64)
            one[(5 * k + 3 * v) % J] = hostile_row(fam, rng, v)
            frames.append(one)
    q = osf._f32(np.stack(frames))
    assert np.isnan(q).any() and np.isinf(q).any() and (q == 0).all(axis=-1).any()
    same(run(f["tr"], q, layout), compose(q, f["src"], f["pre"], f["post"]), (name, layout, "families"))
    if J in (21, 59):
        tag = f"family_{J}"
        same(run(f["tr"], fx[tag], layout), fx[f"out_{tag}_{name}"], (name, layout, "the reference's family frames"))
    else:
        okey = "out_broadcast_23_broadcast" if name == "vtrdyn_broadcast" else "out_broadcast_23_full_scatter"
        same(run(f["tr"], fx["broadcast_23"], layout), fx[okey], (name, layout, "the reference's broadcast batch"))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", FORMS)
def test_one_off_table_row_per_64_items(forms, name, layout):
    """Copies of an ordinary frame; of every 64 consecutive (frame, output joint) items exactly one reads an input row
    whose norm is off the near-unit table, at a moving place: the rare-case branch with one lane in it."""
    f = forms[name]
    B, J_out = 64, f["tr"].J_out
    src = np.arange(J_out) if f["src"] is None else np.asarray(f["src"])
    q = np.repeat(f["q"][:1], B, axis=0).copy()
    for g in range(B * J_out // 64):
        item = 64 * g + (7 * g + 3) % 64
        fr, j = divmod(item, J_out)
        q[fr, src[j]] *= np.float32(1.5)
    hit = (q[:, src] != f["q"][:1, src]).any(axis=2).reshape(-1)   # per item: its input row is an off-table one
    assert (hit.reshape(-1, 64).sum(axis=1) == 1).all()
    same(run(f["tr"], q, layout), compose(q, f["src"], f["pre"], f["post"]), (name, layout))


def _code_scale(c):
    """The factor that moves a unit quaternion's |q|^2 by c float32 codes: a code is 2^-23 above 1.0f and 2^-24 below."""
    c = np.asarray(c, np.float64)
    return np.sqrt(1.0 + c * np.where(c < 0, 2.0 ** -24, 2.0 ** -23))


def _norm_code(p):
    """|p|^2 summed as the kernels sum it, ((x x + y y) + z z) + w w in float32, as its distance in codes from 1.0f."""
    x, y, z, w = (np.ascontiguousarray(p[:, k], np.float32) for k in range(4))
    s = ((x * x + y * y) + z * z) + w * w
    return s.view(np.int32).astype(np.int64) - 0x3F800000


@pytest.mark.parametrize("layout", LAYOUTS)
def test_near_unit_table_edges(gpu, fx, layout):
    """Both products' |p|^2 on the table's last codes (1.0f -+ 16 codes) and on the first codes off it (-+ 17), on many
    items: the inputs and post rows are unit quaternions scaled to a chosen code (_code_scale), and the host checks with the
    oracle's own products that every one of the four codes is met by at least eight items of either product."""
    import oracle as orc
    from rtg import ingest
    J, B = 32, 64
    rng = np.random.default_rng(7800)
    ks = np.array([-18, -17, -16, -15, 15, 16, 17, 18, 0, -17, 17, -16])
    q = osf._f32(rf.unit_rows(rng, (B, J)) * _code_scale(ks[rng.integers(0, len(ks), (B, J))])[..., None])
    pre = np.ascontiguousarray(fx["pre_vtrdyn"], np.float32)
    post = osf._f32(rf.unit_rows(rng, (J,)) * _code_scale(ks[np.arange(J) % len(ks)])[:, None])
    rows, pre_b = q.reshape(-1, 4), np.ascontiguousarray(np.broadcast_to(pre, (B * J, 4)))
    post_b = np.ascontiguousarray(np.broadcast_to(post, (B, J, 4)).reshape(-1, 4))
    c1 = _norm_code(orc.quat_mul(rows, pre_b))
    c2 = _norm_code(orc.quat_mul(orc.quat_mul_norm(rows, pre_b), post_b))
    for c in (c1, c2):
        for code in (-17, -16, 16, 17):
            assert (c == code).sum() >= 8, (code, int((c == code).sum()))
    tr = ingest.ZeroPoseTransform(J, None, pre, post)
    same(run(tr, q, layout), compose(q, None, pre, post), ("table edges", layout))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", FORMS)
def test_single_bad_elements(forms, name, layout):
    """One NaN element, one zero row, one inf, at frames 0, T - 1, T and B - 1: the frame equals the oracle, every other
    frame keeps the clean launch's bits.  For 23 -> 21, NaN in the dropped rows 4 and 8 changes nothing."""
    f = forms[name]
    T = _tile(layout)
    B, J = 3 * T + 5, f["J_in"]
    base = f["q"][:B]
    clean = run(f["tr"], base, layout)
    same(clean, f["want"][:B], (name, layout, "clean"))
    row = 11 % J
    for kind in ("nan", "zero_row", "inf"):
        for fr in (0, T - 1, T, B - 1):
            q = base.copy()
            if kind == "zero_row":
                q[fr, row] = 0.0
            else:
                q[fr, row, fr % 4] = np.nan if kind == "nan" else np.inf
            got = run(f["tr"], q, layout)
            same(got, compose(q, f["src"], f["pre"], f["post"]), (name, layout, kind, fr))
            others = np.arange(B) != fr
            assert np.array_equal(bits(got[others]), bits(clean[others])), (name, layout, kind, fr)
            assert (bits(got[fr]) != bits(clean[fr])).any()
    if J == 23:
        q = base.copy()
        q[:, 4] = np.nan
        q[:, 8, 2] = np.nan
        assert np.array_equal(bits(run(f["tr"], q, layout)), bits(clean)), "a dropped row reached the output"


@pytest.mark.parametrize("layout", LAYOUTS)
def test_generic_shapes(gpu, layout):
    """Random src with repeats, non-unit pre and post, J_in and J_out over {1, 2, 7, 36, 37, 64}, B = 3 T + 5."""
    from rtg import ingest
    B = 3 * _tile(layout) + 5
    rng = np.random.default_rng(7600)
    sizes = (1, 2, 7, 36, 37, 64)
    for J_in in sizes:
        q = osf._f32(rf.unit_rows(rng, (B, J_in)) * rng.uniform(0.5, 2.0, (B, J_in, 1)))
        for J_out in sizes:
            src = rng.integers(0, J_in, J_out)
            if J_out > 1:
                src[-1] = src[0]                                            # a repeat, whatever the draw
            pre = osf._f32(rng.normal(size=4) * 1.7)
            post = osf._f32(rf.unit_rows(rng, (J_out,)) * rng.uniform(0.5, 2.0, (J_out, 1)))
            tr = ingest.ZeroPoseTransform(J_in, src, pre, post)
            same(run(tr, q, layout), compose(q, src, pre, post), (J_in, J_out, layout))
    ident = ingest.ZeroPoseTransform(7, None, pre, post[:7])                # src = None: the identity
    q = rf.unit_frames(B, 7)
    same(run(ident, q, layout), compose(q, None, pre, post[:7]), ("identity", layout))


def test_drop_in_functions_and_device_built_constants(gpu, fx):
    """The module functions carry the reference's names and meaning: CPU tensors in, the reference's recorded outputs
    out, on the CPU; a device tensor stays on the device.  The constants built on the device from the package's assets
    are the reference's."""
    from rtg import ingest
    for asset in ("vtrdyn", "vtrdyn_full"):
        assert np.array_equal(bits(ingest.t2zero_pose_transform_quat(asset)), bits(fx[f"t2zero_{asset}"])), asset
    for name, pre, t2z in (("vtrdyn", "pre_vtrdyn", "t2zero_vtrdyn"), ("vtrdyn_full", "pre_vtrdyn_full", "t2zero_vtrdyn_full"),
                           ("vtrdyn_broadcast", "pre_broadcast", "t2zero_vtrdyn")):
        tr = getattr(ingest.ZeroPoseTransform, name)()
        assert np.array_equal(bits(tr.pre), bits(fx[pre])), name
        if name != "vtrdyn_broadcast":
            assert np.array_equal(bits(tr.post), bits(conj(fx[t2z]))), name
    tr = ingest.ZeroPoseTransform.vtrdyn_full_from_broadcast()
    assert np.array_equal(bits(tr.post), bits(conj(fx["t2zero_vtrdyn_full"])[rf.BODY21_IN_FULL59]))
    assert tr.src.tolist() == rf.BODY23_TO_21
    for fn, ikey, okey in ((ingest.vtrdyn_zero_pose_transform, "family_21", "out_family_21_vtrdyn"),
                           (ingest.zero_pose_transform_quat, "unit_21", "out_unit_21_vtrdyn"),
                           (ingest.vtrdyn_broadcast_zero_pose_transform, "family_21", "out_family_21_broadcast"),
                           (ingest.vtrdyn_full_zero_pose_transform, "family_59", "out_family_59_vtrdyn_full")):
        x = torch.from_numpy(fx[ikey])
        y = fn(x)
        assert y.device.type == "cpu" and y.shape == x.shape
        same(y.numpy(), fx[okey], okey)
        one = fn(x[3])                                                      # a single frame, as the teleop loop calls it
        same(one.numpy(), fx[okey][3], okey + " [3]")
    y = ingest.vtrdyn_zero_pose_transform(torch.from_numpy(fx["unit_21"]).to(gpu))
    assert y.is_cuda
    same(y.cpu().numpy(), fx["out_unit_21_vtrdyn"], "device in, device out")
    same(ingest.ingest_rotations(fx["broadcast_23"]).cpu().numpy(), fx["out_broadcast_23_broadcast"], "ingest_rotations")
    same(ingest.ingest_rotations(fx["broadcast_23"], ingest.ZeroPoseTransform.vtrdyn_full_from_broadcast()).cpu().numpy(),
         fx["out_broadcast_23_full_scatter"], "ingest_rotations, 59-joint constants")
    with pytest.raises(ValueError):
        ingest.ingest_rotations(fx["unit_21"])
    with pytest.raises(ValueError):
        ingest.ZeroPoseTransform.vtrdyn()(fx["unit_59"])


@pytest.mark.parametrize("kind", (osf.BODY_ROT, osf.FULL_BODY_ROT))
def test_through_a_solver(gpu, forms, kind):
    """ingest_rotations(..., layout="soa") feeds the rotation solvers at B = 129; the result is the same solver's on the
    oracle-composed rotations handed over as AoS rows: the planes are the solver's planes."""
    from rtg import assets, ingest, synth
    from rtg.runtime import Solver
    B = 129
    zp = golden("zero_pose")
    asset = "vtrdyn_full" if kind == osf.FULL_BODY_ROT else "vtrdyn"
    S = Solver(kind, zp[f"{asset}_local_t"], zp[f"{asset}_global_t"], assets.parents(asset), False)
    f = forms["vtrdyn_broadcast"]
    raw = f["q"][:B]
    rest = [np.ascontiguousarray(a) for a in synth.synth_full_body_rot_inputs(B, 7700)[1:]] if kind == osf.FULL_BODY_ROT else []
    planes = ingest.ingest_rotations(raw, layout="soa")
    assert tuple(planes.shape) == (21, 4, B)
    soa_in = [planes] + [torch.from_numpy(a).to(gpu).permute(1, 2, 0).contiguous() for a in rest]
    aos_in = [torch.from_numpy(a).to(gpu) for a in [f["want"][:B]] + rest]
    got = S.retarget(soa_in, want_local_rot=True, layout="soa")
    want = S.retarget(aos_in, want_local_rot=True, layout="aos")
    for g, w, what in zip(got[:2], want[:2], ("dof", "local_rot")):
        same(g.cpu().numpy(), w.cpu().numpy(), what)
    assert np.isfinite(want[0].cpu().numpy()).all(axis=1).mean() > 0.9       # the solver solved these frames


def test_launch_argument_checks_with_a_handle(gpu):
    """What the host test cannot reach without a device: overlapping q / out, B = 0, and a misaligned buffer."""
    from rtg import _lib
    lib = _lib.lib()
    ip, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    pre = np.array([0, 0, 0, 1], np.float32)
    post = np.tile(pre, (21, 1))
    src = np.asarray(rf.BODY23_TO_21, np.int32)
    h = ctypes.c_void_p()
    _lib.check(lib.rtg_rot_ingest_create(23, 21, src.ctypes.data_as(ip), pre.ctypes.data_as(fp), post.ctypes.data_as(fp),
                                         ctypes.byref(h)))
    B = 8
    buf = torch.zeros(B * 23 * 4 + B * 21 * 4, device=gpu)
    q, stream = buf.data_ptr(), ctypes.c_void_p()
    try:
        for out, word in ((q, "overlap"), (q + 16 * (B * 23 - 1), "overlap"), (q - 16 * (B * 21 - 1), "overlap"),
                          (q + 16 * B * 23 + 4, "16-byte aligned")):
            for layout in (0, 1):
                rc = lib.rtg_rot_ingest_f32(h, ctypes.c_void_p(q), B, layout, ctypes.c_void_p(out), stream)
                assert rc == 1 and word in lib.rtg_last_error().decode(), (rc, lib.rtg_last_error())
        assert lib.rtg_rot_ingest_f32(h, None, 0, 1, None, stream) == 0           # B = 0: a no-op
        assert lib.rtg_rot_ingest_f32(h, ctypes.c_void_p(q), B, 0, ctypes.c_void_p(q + 16 * B * 23), stream) == 0   # adjacent
        torch.cuda.synchronize()
    finally:
        lib.rtg_rot_ingest_destroy(h)

"""UPPER_BODY, FULL_BODY_ROT and BODY_ROT on hostile input, bit for bit against the C oracle: the 4096 frames per
kind of tests/other_solver_frames.py (non-unit, near-unit, tiny, huge, negated, gimbal-locked, zero, NaN and inf
rotations; the torso-fit families, degenerate arms, rescaled frames and the gripper threshold), in whole 64-frame
waves of one family and mixed within a wave, through ragged batches, a fully resident chip, waves that hold exactly
one rare-path element, and frames that raise next to frames that do not.  tests/test_other_solvers_host.py checks
the oracle-only conditions these tests rest on and anchors the oracle on the same families to the reference.

Every comparison is on the raw bits, every NaN reading alike (tests/test_gpu_edge.py::_bits); the frame codes are
compared exactly through rtg.runtime.frame_status.  The last section runs the two Euler entry points over every
axis sequence, intrinsic and extrinsic.

What these tests found (measured on an MI355X, both layouts, also with RTG_UPPER_UNIT_TAB = RTG_ROT_UNIT_TAB = 0).
UPPER_BODY was bit-exact throughout.  FULL_BODY_ROT differed from the oracle on 13 of its 4096 frames (7
w_table_edges, 6 half_turn) and BODY_ROT on 11 (6 half_turn, 5 w_table_edges), all in links the Euler split writes, on
frames where the oracle agrees with the recorded reference: components below 4e-9 off by at most 3.5e-16, +0 against
-0, and in three FULL_BODY_ROT frames a half-turn link q for the oracle's -q (DOF +pi for -pi).  Cause: scipy_as_euler
(csrc/rtg_math.cuh; every YXZ / ZYX split and every declined XYZ split) took the device library's float64 atan2 and
hypot, whose last bits are not the host libm's: of 2^20 random unit quaternions 31-36 % of rtg_quat_as_euler_f64's
angles differed from the oracle's, by at most 1.8e-15, and an angle half_sum -+ half_diff that cancels to ~1e-16 ..
1e-9 or lands within an ulp of +-pi (the wrap) carries that bit into float32.  Fixed (RTG_EULER_LIBM): hypot as the
host libm computes it (bit-identical on 2e7 arguments) and a correctly rounded atan2; the same probe now differs in
0.08-0.10 % of the angles, which is the host atan2's own misrounding (7.4e-4 of random arguments against a 300-bit
evaluation), and every test below passes.  That remainder can still show in a frame like these; closing it would
take the host's atan2 restated on the device."""
import itertools

import numpy as np
import pytest
import torch

from conftest import golden
from test_gpu_edge import _bits

import other_solver_frames as osf

pytestmark = pytest.mark.gpu

KINDS = sorted(osf.NAMES)
IDS = [osf.NAMES[k] for k in KINDS]
N0 = osf.N0
RAGGED = (1, 63, 64, 65, 127, 128, 129, 128 * 37 + 65)   # the block is 128 frames: two 64-frame tiles
QNAN = 0x7FC00000


def _solver(kind):
    from rtg import assets
    from rtg.runtime import Solver
    zp = golden("zero_pose")
    name = "vtrdyn_full" if kind == osf.FULL_BODY_ROT else "vtrdyn"
    return Solver(kind, zp[f"{name}_local_t"], zp[f"{name}_global_t"], assets.parents(name), False)


def _solved(kind):
    """The kind's N0 frames on the host and on the device, and the oracle's result for them (computed once; a frame's
    result does not depend on its batch, so every batch below indexes into it)."""
    import oracle as orc
    d = osf.frames(kind)
    dof, lr = osf.oracle_run(kind, d)
    ins = tuple(d[k] for k in osf.INPUTS[kind])
    out = dict(kind=kind, ins=ins, dev=[torch.from_numpy(a).cuda() for a in ins], family=d["family"],
               dof_bits=_bits(dof), lr_bits=_bits(lr), status=orc.frame_status(dof))
    for a in (out["dof_bits"], out["lr_bits"], out["status"]):
        a.setflags(write=False)       # shared by every test of the module
    return out


@pytest.fixture(scope="module")
def upper_body(gpu):
    return _solved(osf.UPPER_BODY)


@pytest.fixture(scope="module")
def full_body_rot(gpu):
    return _solved(osf.FULL_BODY_ROT)


@pytest.fixture(scope="module")
def body_rot(gpu):
    return _solved(osf.BODY_ROT)


@pytest.fixture
def solved(request, kind):
    return request.getfixturevalue(osf.NAMES[kind])


def _launch(S, dev, layout, rots):
    if layout == "soa":
        dev = [t.permute(1, 2, 0).contiguous() for t in dev]
    dof, lr, _ = S.retarget(dev, want_local_rot=rots, layout=layout)
    assert (lr is not None) == rots
    return dof, lr


def _where(solved, idx, bad):
    """Names the mismatching rows of a batch: (row, frame, family) of the first few, and the count per family."""
    fams = [f[0] for f in osf.FAMILIES[solved["kind"]]] + ["plain"]
    rows = np.flatnonzero(bad)
    who = [fams[solved["family"][idx[r]]] for r in rows]
    count = {f: who.count(f) for f in dict.fromkeys(who)}
    return f"{len(rows)} of {len(idx)} rows differ, by family {count}; first (row, frame, family): " \
           f"{[(int(r), int(idx[r]), w) for r, w in zip(rows[:6], who)]}"


def _check(S, solved, idx, layout, rots, tag):
    """The frames idx of the fixture as one batch (gathered on the device) against the oracle."""
    from rtg.runtime import frame_status
    idx = np.asarray(idx, np.int64)
    sel = torch.from_numpy(idx).cuda()
    dof, lr = _launch(S, [t[sel].contiguous() for t in solved["dev"]], layout, rots)
    bad = frame_status(dof).cpu().numpy() != solved["status"][idx]
    assert not bad.any(), f"{tag}: status: {_where(solved, idx, bad)}"
    bad = (_bits(dof) != solved["dof_bits"][idx]).any(axis=1)
    if rots:
        bad |= (_bits(lr) != solved["lr_bits"][idx]).any(axis=(1, 2))
    assert not bad.any(), f"{tag}: dof / local_rot bits: {_where(solved, idx, bad)}"


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_families_vs_oracle(solved, kind, layout):
    """All N0 frames in one batch: every family mixed within the first two waves and in a whole wave of its own."""
    _check(_solver(kind), solved, np.arange(N0), layout, True, f"{osf.NAMES[kind]} {layout}")


def _special_frames(solved):
    """(an ordinary frame, a raising frame, a frame of a rare-path family that the oracle solves)."""
    kind, st = solved["kind"], solved["status"]
    ordinary = N0 - 1
    raising = int(osf.wave(kind, "nan_torso" if kind == osf.UPPER_BODY else "zero_row")[5])
    rare = int(osf.wave(kind, "torso_collinear" if kind == osf.UPPER_BODY else "gimbal")[5])
    assert solved["family"][ordinary] < 0 and st[ordinary] == 0 and st[raising] > 0 and st[rare] == 0
    return ordinary, raising, rare


@pytest.mark.parametrize("B", RAGGED)
@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_ragged_batches_vs_oracle(solved, kind, layout, B):
    """Batches that end at, one before and one after a tile's and a block's edge, with and without local rotations.
    Every third tile has a raising frame at its rows 0 and 63; for B = 1, 65 and 129 (a last tile with one live lane)
    that lane is, in turn, an ordinary frame, a raising frame and a frame of a rare-path family."""
    S = _solver(kind)
    ordinary, raising, rare = _special_frames(solved)
    idx = np.arange(B) % N0
    for t in range(0, (B + 63) // 64, 3):
        for p in (64 * t, 64 * t + 63):
            if p < B:
                idx[p] = raising
    lasts = (ordinary, raising, rare) if B in (1, 65, 129) else (None,)
    for last in lasts:
        if last is not None:
            idx[-1] = last
        if B >= 64:
            assert solved["status"][idx[[0, 63]]].all() and (solved["status"][idx] == 0).any()
        for rots in (True, False):
            _check(S, solved, idx, layout, rots, f"{osf.NAMES[kind]} B={B} {layout} rots={rots} last={last}")


def _canon(t):
    """int32 view of a float32 tensor with every NaN reading alike (the device-side _bits)."""
    return torch.where(torch.isnan(t), torch.full((), QNAN, dtype=torch.int32, device=t.device), t.view(torch.int32))


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_full_residency_vs_oracle(solved, kind, layout):
    """One launch that fills every compute unit with as many blocks as the runtime reports resident, and a ragged
    tile: for UPPER_BODY the R10 hand-over with every wave slot taken.  Built on the device by index gather and compared
    there, row by row, with the N0 oracle results uploaded once."""
    from rtg import ops
    from rtg.runtime import frame_status
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = ops.side_kernel_residency(kind, False, layout) * cus * 128 + 65
    sel = torch.arange(B, device="cuda") % N0
    dof, lr = _launch(_solver(kind), [t[sel].contiguous() for t in solved["dev"]], layout, True)
    ref_dof = torch.from_numpy(solved["dof_bits"].view(np.int32)).cuda()
    ref_lr = torch.from_numpy(solved["lr_bits"].view(np.int32)).cuda()
    ref_st = torch.from_numpy(solved["status"].astype(np.int64)).cuda()
    assert torch.equal(frame_status(dof).to(torch.int64), ref_st[sel]), "status"
    assert torch.equal(_canon(dof), ref_dof[sel]), "dof"
    assert torch.equal(_canon(lr), ref_lr[sel]), "local_rot"


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_one_rare_element_per_group(gpu, kind):
    """Copies of one ordinary frame, and in every 64-frame wave exactly one frame that differs from it in a single
    rare-path element (one gimbal-locked joint, one link whose w sits on an angle-table edge, one row whose squared
    norm is on, at the edge of or off the near-unit table, a degenerate arm or torso; the left or the right side only)
    at a lane that moves from wave to wave.  The ordinary copies keep the ordinary frame's bits, the rare frames equal
    the oracle, both layouts."""
    import oracle as orc
    from rtg.runtime import frame_status
    base, rare = osf.rare_frames(kind)
    keys = osf.INPUTS[kind]
    uniq = {k: np.stack([base[i]] + [f[i] for _, f in rare]) for i, k in enumerate(keys)}
    odof, olr = osf.oracle_run(kind, uniq)
    ost = orc.frame_status(odof)
    assert ost[0] == 0 and np.isfinite(odof[0]).all()
    changed = (_bits(odof[1:]) != _bits(odof[:1])).any(axis=1)
    assert changed.mean() > 0.5                       # the rare element reaches the DOFs of most frames
    idx = np.zeros(64 * len(rare), np.int64)
    lanes = (np.arange(len(rare)) * 7 + 3) % 64
    idx[64 * np.arange(len(rare)) + lanes] = 1 + np.arange(len(rare))
    assert ((idx.reshape(-1, 64) != 0).sum(axis=1) == 1).all()
    S = _solver(kind)
    sel = torch.from_numpy(idx).cuda()
    dev = [torch.from_numpy(uniq[k]).cuda()[sel].contiguous() for k in keys]
    for layout in ("aos", "soa"):
        dof, lr = _launch(S, dev, layout, True)
        got_d, got_l = _bits(dof), _bits(lr)
        plain = idx == 0
        assert (got_d[plain] == _bits(odof[0])).all() and (got_l[plain] == _bits(olr[0])).all(), \
            f"{layout}: an ordinary copy lost its bits beside a rare frame"
        bad = [rare[i - 1][0] for i in idx[~plain] if not ((got_d[idx == i] == _bits(odof[i])).all()
                                                           and (got_l[idx == i] == _bits(olr[i])).all())]
        assert not bad, f"{layout}: rare frames off the oracle: {bad[:8]} ({len(bad)} of {len(rare)})"
        np.testing.assert_array_equal(frame_status(dof).cpu().numpy(), ost[idx])


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_frames_are_isolated(solved, kind):
    """A NaN frame and a zero-quaternion frame (UPPER_BODY: an inf torso point) in the middle of a tile of ordinary
    frames: both are marked, every other row keeps the bits of the clean run, and two runs give the same bits."""
    from rtg.runtime import frame_status
    S = _solver(kind)
    n = 3 * 64 + 17
    first = N0 - n
    assert (solved["family"][first:] < 0).all()
    clean = [t[first:].clone() for t in solved["dev"]]
    dirty = [t.clone() for t in clean]
    a, b = 31, 64 + 40
    if kind == osf.UPPER_BODY:
        dirty[0][a, 13, 1] = float("nan")
        dirty[0][b, 11, 2] = float("inf")
    else:
        dirty[0][a, 18 if kind == osf.BODY_ROT else 20, 2] = float("nan")
        dirty[0][b, 14 if kind == osf.BODY_ROT else 13] = 0.0
    for layout in ("aos", "soa"):
        dof0, lr0 = _launch(S, clean, layout, True)
        dof1, lr1 = _launch(S, dirty, layout, True)
        dof2, lr2 = _launch(S, dirty, layout, True)
        assert torch.equal(_canon(dof1), _canon(dof2)) and torch.equal(_canon(lr1), _canon(lr2))
        assert torch.equal(dof1.view(torch.int32)[:, 0], dof2.view(torch.int32)[:, 0])   # the codes, bit for bit
        st = frame_status(dof1).cpu().numpy()
        assert st[a] > 0 and st[b] > 0 and st.sum() == st[a] + st[b] and not frame_status(dof0).any()
        assert torch.isnan(dof1[[a, b]]).all() and torch.isnan(lr1[[a, b]]).all()
        keep = torch.ones(n, dtype=torch.bool, device="cuda")
        keep[[a, b]] = False
        assert torch.equal(dof1[keep].view(torch.int32), dof0[keep].view(torch.int32))
        assert torch.equal(lr1[keep].view(torch.int32), lr0[keep].view(torch.int32))
        np.testing.assert_array_equal(_bits(dof0), solved["dof_bits"][first:])


# ---- the Euler entry points over every axis sequence (on the solver path only XYZ, YXZ, ZYX and xyz ever run)
SEQS = ["".join(s) for s in itertools.product("XYZ", repeat=3) if s[0] != s[1] and s[1] != s[2]]
SEQS = SEQS + [s.lower() for s in SEQS]


def _euler_inputs(seq):
    """257 quaternions (a ragged second block): random unit (either sign of w), non-unit, gimbal-locked for seq (middle
    angle 0 or pi for a symmetric sequence, +-pi / 2 otherwise; exact in float64, rounded to float32), one zero row and
    one NaN row."""
    rng = np.random.default_rng(sum(map(ord, seq)) * 7 + seq.islower())
    n = 257
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[64:128] *= rng.uniform(0.5, 2.0, (64, 1))
    mids = (0.0, np.pi) if seq[0] == seq[2] else (np.pi / 2, -np.pi / 2)
    for i in range(128, 224):
        ang = (rng.uniform(-np.pi, np.pi), mids[i % 2], rng.uniform(-np.pi, np.pi))
        s, a = (seq, ang) if seq.isupper() else (seq.upper()[::-1], ang[::-1])   # extrinsic abc = intrinsic cba
        q[i] = osf.euler_quat(s, a) * (1.0 if i % 4 < 2 else -1.0)
    q = q.astype(np.float32)
    q[230] = 0.0
    q[256, 1] = np.nan
    return q


@pytest.mark.parametrize("seq", SEQS)
def test_euler_entry_points_every_sequence(gpu, seq):
    """rtg_quat_in_xyz_axis_f32 against the oracle bit for bit, rtg_quat_as_euler_f64 (radians and degrees) within the
    tolerance test_rotation3d_transform3d_full_surface_vs_oracle_and_reference uses for xyz; the zero and the NaN row
    are refused and carry the marked NaN (rtg.h RTG_FRAME_ZERO_NORM_QUAT in the payload)."""
    import oracle as orc
    from rtg import ops
    q = _euler_inputs(seq)
    dq = torch.from_numpy(q).cuda()
    want = orc.quat_in_xyz_axis(q, seq)
    got = torch.stack(ops.quat_in_xyz_axis(dq, seq), dim=1).cpu().numpy()
    refused = np.zeros(len(q), bool)
    refused[[230, 256]] = True
    np.testing.assert_array_equal(got.view(np.uint32)[refused], np.uint32(QNAN | 2))
    np.testing.assert_array_equal(want.view(np.uint32)[refused], np.uint32(QNAN | 2))
    assert not np.isnan(got[~refused]).any()
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    eu = orc.as_euler(q, seq)
    # the gimbal rows reach scipy's degenerate branch (an angle it zeroes) in this sequence
    assert (eu[128:224][:, 2] == 0.0).any()
    for degrees in (False, True):
        e = ops.quat_as_euler(dq, seq, degrees=degrees).cpu().numpy()
        np.testing.assert_array_equal(e.view(np.uint64)[refused], np.uint64(0x7FF8000000000002))
        ref = eu * (180.0 / np.pi) if degrees else eu
        np.testing.assert_allclose(e[~refused], ref[~refused], rtol=1e-13, atol=1e-12)


def test_euler_angles_last_bits_vs_host_libm(gpu):
    """rtg_quat_as_euler_f64's angles against the oracle's bit for bit on 2^18 random unit quaternions.  The device
    computes hypot as the host libm does and atan2 correctly rounded; the host's atan2 misrounds 7.4e-4 of random
    arguments (measured against a 300-bit evaluation), and an angle takes at most two atan2 calls, so at most 2 * 7.4e-4
    of the rows may differ per angle, by a few ulps of pi.  (The device library's own atan2 / hypot gave 31-36 %.)"""
    import oracle as orc
    from rtg import ops
    rng = np.random.default_rng(3)
    q = rng.normal(size=(1 << 18, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    for seq in ("YXZ", "ZYX", "XYZ", "xyz"):
        d = ops.quat_as_euler(torch.from_numpy(q).cuda(), seq).cpu().numpy()
        o = orc.as_euler(q, seq)
        frac = (d.view(np.int64) != o.view(np.int64)).mean(axis=0)
        print(seq, "fraction of angles whose float64 bits differ:", frac, "max |diff|", np.abs(d - o).max())
        assert (frac <= 2 * 7.4e-4).all(), (seq, frac)
        assert np.abs(d - o).max() <= 4 * 2.0 ** -51


# ---- FULL_BODY_POS: the declined XYZ split through every kernel that serves it
@pytest.fixture(scope="module")
def fbp_wrists(gpu):
    import oracle as orc
    zp = golden("zero_pose")
    ins = osf.fbp_wrist_frames()
    dof, lr, br = orc.full_body_pos(zp["vtrdyn_full_local_t"], zp["vtrdyn_full_global_t"], *ins, True)
    assert not orc.frame_status(dof).any()
    return dict(dev=[torch.from_numpy(a).cuda() for a in ins], ref=[_bits(a) for a in (dof, lr, br)], lr=lr)


def test_fbp_wrist_frames_are_single_axis(fbp_wrists):
    """The oracle alone: in nine frames of ten, two of the wrist's three Euler links (16-18 left, 25-27 right) are the
    identity or a half turn up to 1e-5 (the float32 rounding of the hand points, ~6e-8 m over ~5 cm): a sine or cosine
    that small is the component whose float32 value a last float64 bit of the split's atan2 decides."""
    lr = fbp_wrists["lr"]
    for l0 in (16, 25):
        e = lr[:, l0:l0 + 3]
        tiny = np.minimum(np.abs(e[..., :3]).max(axis=2), np.abs(e[..., 3])) < 1e-5
        assert (tiny.sum(axis=1) >= 2).mean() > 0.9


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_fbp_declined_euler_split_every_kernel(fbp_wrists, layout):
    """FULL_BODY_POS frames whose wrist-local rotation is a single-axis rotation (identity, half turns, w edges) up to
    the Kabsch fit's rounding, through k_fbp_frame1 (B = 1, 48 launches), k_fbp_quad (B = 512), k_fbp_latency5
    (B = 4096 + 65) and k_solve_sides (B = 49152 + 65): DOFs, local and body rotations equal the oracle's bits, hence
    each other's.  The lane-parallel restatement of the split (the two small-batch kernels) and the per-lane one (the
    other two) must take the same atan2 / hypot."""
    from rtg import _lib, assets
    from rtg.runtime import Solver
    zp = golden("zero_pose")
    S = Solver(_lib.SOLVER_FULL_BODY_POS, zp["vtrdyn_full_local_t"], zp["vtrdyn_full_global_t"],
               assets.parents("vtrdyn_full"), True)
    n = osf.FBP_WRIST_N
    got = {}
    for B in (n, 4096 + 65, 49152 + 65):
        sel = torch.arange(B, device="cuda") % n
        dev = [t[sel].contiguous() for t in fbp_wrists["dev"]]
        if layout == "soa":
            dev = [t.permute(1, 2, 0).contiguous() for t in dev]
        out = S.retarget(dev, want_local_rot=True, want_body_rot=True, layout=layout)
        idx = sel.cpu().numpy()
        bad = np.zeros(B, bool)
        for o, r in zip(out, fbp_wrists["ref"]):
            bad |= (_bits(o) != r[idx]).reshape(B, -1).any(axis=1)
        assert not bad.any(), f"B={B} {layout}: {int(bad.sum())} rows off the oracle, first frames {idx[bad][:8]}"
        got[B] = [_bits(o)[:n] for o in out]
    for B in (4096 + 65, 49152 + 65):
        for a, b in zip(got[n], got[B]):
            np.testing.assert_array_equal(a, b)
    off = []
    for i in range(48):
        dev = [t[i:i + 1].contiguous() for t in fbp_wrists["dev"]]
        if layout == "soa":
            dev = [t.permute(1, 2, 0).contiguous() for t in dev]
        out = S.retarget(dev, want_local_rot=True, want_body_rot=True, layout=layout)
        if any((_bits(o) != r[i:i + 1]).any() for o, r in zip(out, fbp_wrists["ref"])):
            off.append(i)
    assert not off, f"B=1 {layout}: frames off the oracle {off}"

"""The side kernel (k_solve_sides) with its hand-over slot inside the frame's own DOF row (the row's first four dwords,
fixed zeros of the result) and the SoA FULL_BODY_POS instantiation at five workgroups per compute unit: ragged last
tiles, frames the reference raises on at the tile's edge rows, every compute unit fully resident, the other solver
kinds that share the kernel's shared-memory arrays, and the residency the runtime reports.  Every value is compared bit
for bit against the C oracle; NaNs compare as NaN (test_gpu_torso_fit.py's rule)."""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

N0 = 2048                       # distinct frames, a multiple of the 64-frame tile: frame i sits in tile row (i % N0) % 64
SIDE0 = 49152                   # the largest small-batch size; the side kernel starts one above
BATCHES = (SIDE0 + 1, SIDE0 + 64, SIDE0 + 65, SIDE0 + 128)
FULL_B = 163840 + 65            # 1281 blocks of 128 frames: five blocks on each of 256 compute units, and a ragged tile
# frames the reference raises on: a NaN point in (torso | left wrist | right wrist | torso and both wrists), each at tile
# rows 0 and 63
CASES = ("torso", "left", "right", "all")
RAISING = {name: (64 * (2 * k), 64 * (2 * k + 1) + 63) for k, name in enumerate(CASES)}   # rows 0 and 63 of own tiles


def _bits(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


@pytest.fixture(scope="module")
def frames(gpu):
    """N0 synthetic frames, eight of them with a NaN point, and the oracle's result for them (computed once; a frame's
    result does not depend on its batch, so every batch below indexes into it)."""
    import oracle as orc
    from rtg import assets, ops
    from rtg.runtime import Topology
    zp = golden("zero_pose")
    T = Topology(assets.parents("vtrdyn_full"), assets.local_translation("vtrdyn_full"), assets.tree_quat("vtrdyn_full"))
    body, lh, rh = (t.cpu().numpy() for t in ops.synth_full_body(T, N0, seed=808))
    for name, rows in RAISING.items():
        for i in rows:
            if name in ("torso", "all"):
                body[i, 13, 1] = np.nan      # a torso-fit point
            if name in ("left", "all"):
                lh[i, 6, 2] = np.nan         # a wrist-fit point
            if name in ("right", "all"):
                rh[i, 10, 0] = np.nan
    odof, olr, obr = orc.full_body_pos(zp["vtrdyn_full_local_t"], zp["vtrdyn_full_global_t"], body, lh, rh, True)
    return dict(ins=(body, lh, rh), ref=(odof, olr, obr), status=orc.frame_status(odof))


def _solver():
    from rtg import _lib, assets
    from rtg.runtime import Solver
    zp = golden("zero_pose")
    return Solver(_lib.SOLVER_FULL_BODY_POS, zp["vtrdyn_full_local_t"], zp["vtrdyn_full_global_t"],
                  assets.parents("vtrdyn_full"), True)


def _check(S, frames, idx, layout, rots, tag):
    from rtg.runtime import frame_status
    sel = torch.from_numpy(idx).cuda()
    dev = [torch.from_numpy(a).cuda()[sel].contiguous() for a in frames["ins"]]
    if layout == "soa":
        dev = [t.permute(1, 2, 0).contiguous() for t in dev]
    dof, lr, br = S.retarget(dev, want_local_rot=rots, want_body_rot=rots, layout=layout)
    np.testing.assert_array_equal(frame_status(dof).cpu().numpy(), frames["status"][idx], err_msg=f"{tag}: status")
    np.testing.assert_array_equal(_bits(dof.cpu().numpy()), _bits(frames["ref"][0])[idx], err_msg=f"{tag}: dof")
    if rots:
        np.testing.assert_array_equal(_bits(lr.cpu().numpy()), _bits(frames["ref"][1])[idx], err_msg=f"{tag}: local_rot")
        np.testing.assert_array_equal(_bits(br.cpu().numpy()), _bits(frames["ref"][2])[idx], err_msg=f"{tag}: body_rot")
    else:
        assert lr is None and br is None


def test_oracle_raises_where_planned_and_rarely(frames):
    """The oracle alone: it raises (the SVD's code) on exactly the eight planned frames -- under 5 % -- whose rows are
    all NaN, and every planned case sits at tile rows 0 and 63."""
    st, odof = frames["status"], frames["ref"][0]
    planned = sorted(i for rows in RAISING.values() for i in rows)
    assert {i % 64 for i in planned} == {0, 63} and len(planned) == 2 * len(CASES)
    assert all({i % 64 for i in rows} == {0, 63} for rows in RAISING.values())
    np.testing.assert_array_equal(np.flatnonzero(st), planned)
    assert (st[planned] == 1).all()
    assert (st > 0).mean() < 0.05
    assert np.isnan(odof[planned]).all() and np.isfinite(np.delete(odof, planned, axis=0)).all()


@pytest.mark.parametrize("rots", [True, False], ids=["dof_lr_br", "dof_only"])
@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("B", BATCHES)
def test_ragged_batches_vs_oracle(frames, B, layout, rots):
    """The smallest side-kernel batches: a last block with one live lane and a dead second tile (49153), a whole first
    tile (+64), one live lane in the second tile (+65), a whole block (+128).  The raising frames recur every N0
    frames at rows 0 and 63; for B = 49153 the ragged tile's only live row is, in turn, each raising case."""
    S = _solver()
    idx = np.arange(B) % N0
    if B == SIDE0 + 1:
        for name in CASES:
            idx[-1] = RAISING[name][0]
            assert frames["status"][idx[-1]] == 1
            _check(S, frames, idx, layout, rots, f"B={B} {layout} last={name}")
    else:
        assert frames["status"][idx[SIDE0:]].any()   # the last block holds raising frames too
        _check(S, frames, idx, layout, rots, f"B={B} {layout}")


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_full_residency_vs_oracle(frames, layout):
    """One launch of 1281 blocks on an idle chip: every compute unit holds as many blocks as fit (five for SoA), so the
    hand-overs run with all of a CU's LDS and wave slots taken."""
    _check(_solver(), frames, np.arange(FULL_B) % N0, layout, True, f"B={FULL_B} {layout}")


OTHER = {1: ("upper_body", ("x",)), 2: ("full_body_rot", ("body_rot", "body_pos", "lh", "rh")), 3: ("body_rot", ("global_rot",))}


def _other_oracle(kind, d):
    import oracle as orc
    from rtg import assets
    zp = golden("zero_pose")
    if kind == 1:
        return orc.upper_body(zp["vtrdyn_local_t"], d["x"])
    if kind == 2:
        return orc.full_body_rot(zp["vtrdyn_full_local_t"], d["body_rot"], d["body_pos"], d["lh"], d["rh"])
    return orc.body_rot(assets.parents("vtrdyn"), d["global_rot"])


@pytest.mark.parametrize("kind", [1, 2, 3], ids=["upper_body", "full_body_rot", "body_rot"])
def test_other_kinds_share_the_tile(gpu, kind):
    """UPPER_BODY (it hands R10 over through the same slot), FULL_BODY_ROT and BODY_ROT run k_solve_sides at every
    batch size: B = 1 (the smallest; an ordinary frame, then one the reference raises on), and 128 + 65 (two blocks, a
    ragged second tile whose only live row raises) of the golden frames followed by the edge frames, both layouts, DOFs
    and local rotations."""
    from rtg import _lib, assets
    from rtg.runtime import Solver, frame_status
    import oracle as orc
    name, keys = OTHER[kind]
    zp = golden("zero_pose")
    d = {k: np.concatenate([golden(name)[k], golden(name + "_edge")[k]]) for k in keys}
    odof, olr = _other_oracle(kind, d)
    status = orc.frame_status(odof)
    assert status.any() and (status == 0).any()
    if kind == 2:
        S = Solver(kind, zp["vtrdyn_full_local_t"], zp["vtrdyn_full_global_t"], assets.parents("vtrdyn_full"), False)
    else:
        S = Solver(kind, zp["vtrdyn_local_t"], zp["vtrdyn_global_t"], assets.parents("vtrdyn"), False)
    n = len(odof)
    last = int(np.flatnonzero(status)[-1])
    for B, end in ((1, 0), (1, last), (128 + 65, last)):
        idx = (np.arange(B) + end + 1 - B) % n   # ends on frame `end`: the ragged tile's only live row raises
        assert (status[idx[-1]] != 0) == (end == last) and (B == 1 or (status[idx] == 0).any())
        for layout in ("aos", "soa"):
            dev = [torch.from_numpy(np.ascontiguousarray(d[k][idx])).cuda() for k in keys]
            if layout == "soa":
                dev = [t.permute(1, 2, 0).contiguous() for t in dev]
            dof, lr, _ = S.retarget(dev, want_local_rot=True, layout=layout)
            tag = f"{name} B={B} {layout}"
            np.testing.assert_array_equal(frame_status(dof).cpu().numpy(), status[idx], err_msg=tag)
            np.testing.assert_array_equal(_bits(dof.cpu().numpy()), _bits(odof)[idx], err_msg=tag)
            np.testing.assert_array_equal(_bits(lr.cpu().numpy()), _bits(olr)[idx], err_msg=tag)


# blocks per compute unit that the runtime reported on an MI355X for the build before this layout (its k_solve_sides with
# only the entry point added), by (kind, precise gripper, layout)
PARENT_RESIDENCY = {(0, False, "aos"): 4, (0, False, "soa"): 4, (0, True, "aos"): 4, (0, True, "soa"): 4,
                    (1, False, "aos"): 4, (1, False, "soa"): 4, (2, False, "aos"): 4, (2, False, "soa"): 4,
                    (3, False, "aos"): 5, (3, False, "soa"): 5}


def test_residency_reported(gpu):
    """rtg_side_kernel_residency: FULL_BODY_POS on SoA inputs keeps at least five 256-thread blocks per compute unit
    (five waves per SIMD), and no instantiation reports less than the build before this layout did: FULL_BODY_POS 4
    (both layouts and gripper modes), UPPER_BODY 4, FULL_BODY_ROT 4, BODY_ROT 5 (PARENT_RESIDENCY).  A build whose
    knobs ask for something else (RTG_SIDES_SOA_WAVES below 5, one tile per block: A/B variants) is held to what it
    asks for."""
    from rtg import _lib, ops
    knobs = _lib.build_info()["knobs"]
    got = {}
    for kind in range(4):
        for precise in ((False, True) if kind == 0 else (False,)):
            for layout in ("aos", "soa"):
                got[(kind, precise, layout)] = ops.side_kernel_residency(kind, precise, layout)
    print("side-kernel residency (blocks per CU):", got)
    if knobs["RTG_SIDES_SOA_WAVES"] >= 5 and knobs["RTG_SIDES_TILES"] == 2:
        assert got[(0, True, "soa")] >= 5 and got[(0, False, "soa")] >= 5, got
    if knobs["RTG_SIDES_TILES"] == 2:
        for key, before in PARENT_RESIDENCY.items():
            assert got[key] >= before, (key, got[key], before)
    with pytest.raises(Exception):
        ops.side_kernel_residency(7, False, "aos")

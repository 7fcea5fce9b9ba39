"""The FULL_BODY_POS side kernel's per-side program (k_solve_sides: each wave runs its own side -- wrist fit, arm chain,
Euler split, gripper, read-out -- from one code copy with wave-uniform selects; only the torso quaternion R10 crosses
between the waves, through the DOF row's first four dwords), bit for bit against the C oracle.  NaNs compare as NaN
(test_gpu_torso_fit.py's rule).

The side kernel is reached only above RTG_LATENCY_MAX_B, so the batches are the smallest that reach it: 49152 + 1 (one
live row, a dead second tile), + 65 (one live row in the second tile), + 129 (one live row in a new block).  Every
frame is independent of its batch, so the oracle runs once per (zero pose, gripper mode) on a pool of distinct frames
and a batch is an index map into the pool; comparisons run on the device."""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

LAT = 49152                     # RTG_LATENCY_MAX_B (asserted below)
EXTRAS = (1, 65, 129)
BMAX = LAT + EXTRAS[-1]
N0 = 2048                       # ordinary frames of the pool; the specials follow
NAN32 = 0x7FC00000
SLOT_COLS = list(range(11)) + [29]   # the fixed DOFs: the hand-over slot is 0-3, the left wave writes 4-10 and 29

# ---- the specials of the pool: (name, what is overwritten)
KINDS = ("torso", "left", "right", "all")          # which fits see a NaN point: the reference raises there
SPECIALS = [f"nan_{k}" for k in KINDS] + ["inf_torso", "huge_torso"]
SP = {name: N0 + i for i, name in enumerate(SPECIALS)}
NPOOL = N0 + len(SPECIALS)


def _rand_rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _mirror(body, lh, rh):
    """The frame seen in a mirror (y -> -y) with left and right exchanged: arm joints 18-20 <-> 14-16, torso points
    17 <-> 13, the hands swapped.  A swapped per-side constant or link base makes such a pair of frames disagree."""
    m = np.array([1.0, -1.0, 1.0], np.float32)
    b = body.copy()
    b[:, [18, 19, 20, 14, 15, 16, 17, 13]] = body[:, [14, 15, 16, 18, 19, 20, 13, 17]]
    return b * m, rh * m, lh * m


def _pool():
    """NPOOL frames: the 512 golden frames; 512 of them rigidly rotated (R10 far from identity) with jitter; the mirror
    images of those; 512 more rotations; then the specials."""
    g = golden("full_body_pos_precise")
    rng = np.random.default_rng(2121)
    k = np.arange(N0) % 512
    body, lh, rh = (np.ascontiguousarray(g[n][k]).astype(np.float32) for n in ("body", "lh", "rh"))
    for i in list(range(512, 1024)) + list(range(1536, N0)):
        R = _rand_rot(rng).astype(np.float32)
        for a in (body, lh, rh):
            a[i] = (a[i] @ R.T + rng.normal(0.0, 1e-3, a[i].shape)).astype(np.float32)
    body[1024:1536], lh[1024:1536], rh[1024:1536] = _mirror(body[512:1024], lh[512:1024], rh[512:1024])
    sp = [a[700:700 + len(SPECIALS)].copy() for a in (body, lh, rh)]   # rotated frames as the specials' base
    for i, name in enumerate(SPECIALS):
        if name in ("nan_torso", "nan_all"):
            sp[0][i, 17, 1] = np.nan
        if name in ("nan_left", "nan_all"):
            sp[1][i, 6, 2] = np.nan
        if name in ("nan_right", "nan_all"):
            sp[2][i, 10, 0] = np.nan
        if name == "inf_torso":
            sp[0][i, 13, 0] = np.inf        # inf * (Zt.x = 0) is a NaN in A: off the x0 path, and the reference raises
        if name == "huge_torso":
            sp[0][i, 11, 2] = 1e30          # |M| >= 2^60: off the x0 path, no raise
    return tuple(np.concatenate([a, s]) for a, s in zip((body, lh, rh), sp))


# ---- where the specials sit in a batch (positions; a block is 128 rows: tile 0 rows 0-63, tile 1 rows 64-127)
def _plan():
    pos = {}
    for j, kind in enumerate(KINDS):
        pos[128 * (10 + j) + 64 * (j & 1)] = SP[f"nan_{kind}"]               # row 0 of a tile
        pos[128 * (20 + j) + 64 * (1 - (j & 1)) + 63] = SP[f"nan_{kind}"]    # row 63 of a tile
    # mixed torso paths in one block: tile 0's left wave falls back to the general fit, tile 1's stays on x0; then swapped
    pos[128 * 30 + 5] = SP["inf_torso"]
    pos[128 * 31 + 64 + 5] = SP["inf_torso"]
    pos[128 * 32 + 9] = SP["huge_torso"]
    pos[128 * 33 + 64 + 9] = SP["huge_torso"]
    # the batch's last block, so the ragged tiles see a rotated frame and its mirror image
    pos[LAT] = 600
    pos[LAT + 64] = 600 + 512
    pos[LAT + 128] = 1900
    return pos


def _index():
    idx = np.arange(BMAX) % N0
    for p, s in _plan().items():
        idx[p] = s
    return idx


def _zero_pose(name):
    """shipped; asym: the right shoulder, elbow and hand zero vectors scaled and rotated differently from the left's;
    asym_x: the same with one torso zero vector given a nonzero x, so every frame takes the general torso fit."""
    zp = golden("zero_pose")
    zl = zp["vtrdyn_full_local_t"].astype(np.float32).copy()
    if name != "shipped":
        rng = np.random.default_rng(77)
        for rows, scale in (([38], 1.3), ([39], 0.8), ([41, 45, 49, 53, 56], 1.7)):
            zl[rows] = ((zl[rows] @ _rand_rot(rng).T) * scale).astype(np.float32)
        if name == "asym_x":
            assert (zl[[11, 36, 34], 0] == 0).all()
            zl[36, 0] = np.float32(0.0123)
    return zl, zp["vtrdyn_full_global_t"]


def _canon(t):
    """f32 tensor -> its bits with every NaN alike (NaN sign / payload from arithmetic differs between hosts)."""
    bits = t.contiguous().view(torch.int32)
    return torch.where(torch.isnan(t), torch.full_like(bits, NAN32), bits)


_cache = {}


def _reference(pose, precise):
    """The oracle's pool result for (zero pose, gripper mode) as device bit tensors, and the status; computed once."""
    key = (pose, precise)
    if key not in _cache:
        import oracle as orc
        zl, zg = _zero_pose(pose)
        odof, olr, obr = orc.full_body_pos(zl, zg, *_pool(), precise)
        _cache[key] = dict(bits=tuple(_canon(torch.from_numpy(a).cuda()) for a in (odof, olr, obr)),
                           status=orc.frame_status(odof))
    return _cache[key]


def _inputs():
    if "ins" not in _cache:
        idx = torch.from_numpy(_index()).cuda()
        _cache["idx"] = idx
        _cache["ins"] = tuple(torch.from_numpy(a).cuda()[idx] for a in _pool())
    return _cache["ins"], _cache["idx"]


def _solver(pose, precise):
    from rtg import _lib, assets
    from rtg.runtime import Solver
    zl, zg = _zero_pose(pose)
    return Solver(_lib.SOLVER_FULL_BODY_POS, zl, zg, assets.parents("vtrdyn_full"), precise)


def _run(S, ins, layout, rot):
    dev = [t.contiguous() for t in ins]
    if layout == "soa":
        dev = [t.permute(1, 2, 0).contiguous() for t in dev]
    out = S.retarget(dev, want_local_rot=rot, want_body_rot=rot, layout=layout)
    torch.cuda.synchronize()
    return out


def _same(got, want, tag):
    bad = (_canon(got) != want).reshape(len(got), -1).any(1)
    if bool(bad.any()):
        rows = torch.nonzero(bad).flatten()
        r = int(rows[0])
        cols = torch.nonzero((_canon(got[r]) != want[r]).flatten()).flatten().tolist()
        pytest.fail(f"{tag}: {len(rows)} rows differ from the oracle, first row {r} (block {r // 128}, tile row {r % 64}), "
                    f"elements {cols[:12]}")


def _check(S, ref, ins, idx, layout, rot, tag, rows=slice(None)):
    from rtg.runtime import frame_status
    dof, lr, br = _run(S, ins, layout, rot)
    st = frame_status(dof).cpu().numpy()
    want_st = ref["status"][idx.cpu().numpy()]
    np.testing.assert_array_equal(st[rows], want_st[rows], err_msg=f"{tag}: status")
    _same(dof[rows], ref["bits"][0][idx][rows], f"{tag}: dof")
    if rot:
        _same(lr[rows], ref["bits"][1][idx][rows], f"{tag}: local_rot")
        _same(br[rows], ref["bits"][2][idx][rows], f"{tag}: body_rot")
    # the slot: the right wave's clear landed and the left wave wrote nothing there after its signal, so every frame
    # the reference returns a result for has +0 in the fixed DOFs, bit for bit (from the output alone)
    ok = torch.from_numpy(want_st == 0).cuda()
    fixed = dof.view(torch.int32)[:, SLOT_COLS][ok]
    assert int((fixed != 0).sum()) == 0, f"{tag}: a fixed DOF of a live frame is not +0"
    return dof


def test_the_plan_raises_exactly_where_planned(gpu):
    """From the oracle alone: the reference raises on exactly the planned frames -- the NaN specials (status 1, its
    SVD) and the non-finite torso lane -- in every zero pose; they stay under 5 % of each batch; rows 0 and 63 of
    both tiles are covered; and the rotated frames' R10 is far from identity."""
    from rtg import _lib
    assert _lib.build_info()["knobs"]["RTG_LATENCY_MAX_B"] == LAT
    raising = sorted(SP[n] for n in SPECIALS if n != "huge_torso")
    for pose in ("shipped", "asym", "asym_x"):
        for precise in (True, False):
            st = _reference(pose, precise)["status"]
            assert np.flatnonzero(st).tolist() == raising, (pose, precise)
            assert (st[[SP[f"nan_{k}"] for k in KINDS]] == 1).all()   # the inf lane: 1, or 2 where Zt.x != 0 (asym_x)
    idx = _index()
    planned = np.isin(idx, raising)
    for extra in EXTRAS:
        assert 0 < planned[:LAT + extra].sum() < 0.05 * (LAT + extra)
    for tile in (0, 1):
        assert {0, 63} <= {int(p) % 64 for p in np.flatnonzero(planned) if (p % 128) // 64 == tile}
    obr = _reference("shipped", True)["bits"][2].view(torch.float32)[:, 10]   # body_rot row 10 is R10
    assert float(obr[512:1024, 3].abs().median()) < 0.9


@pytest.mark.parametrize("rot", [False, True], ids=["dofs", "rots"])
@pytest.mark.parametrize("precise", [True, False], ids=["precise", "binary"])
@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("extra", EXTRAS)
def test_side_program_vs_oracle(gpu, extra, layout, precise, rot):
    """Every output of the shipped zero pose: ordinary, rotated and mirrored frames, frames the reference raises on in
    rows 0 and 63 (status and poisoned rows equal the oracle's, the neighbouring rows are untouched), a block whose
    tiles take different torso paths, and the ragged last block."""
    ins, idx = _inputs()
    B = LAT + extra
    _check(_solver("shipped", precise), _reference("shipped", precise), tuple(t[:B] for t in ins), idx[:B], layout, rot,
           f"B={B} {layout}")


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("pose", ["asym", "asym_x"])
def test_asymmetric_zero_pose_vs_oracle(gpu, pose, layout):
    """Per-side selects: the right side's zero vectors differ from the left's in scale and direction (asym), and one
    torso zero vector has a nonzero x so the left wave runs the general torso fit on every frame (asym_x); the oracle
    takes the same zero pose.  The pool holds mirror-image pairs of frames."""
    ins, idx = _inputs()
    ref, base = _reference(pose, True), _reference("shipped", True)
    live = torch.from_numpy(ref["status"] == 0).cuda()
    assert bool((ref["bits"][0][live][:, 20:29] != base["bits"][0][live][:, 20:29]).any(1).float().mean() > 0.9), \
        "the asymmetric zero pose does not move the right side's DOFs"
    _check(_solver(pose, True), ref, ins, idx, layout, True, f"{pose} {layout}")


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_mixed_torso_paths_in_one_block(gpu, layout):
    """Blocks 30-33: one lane of one tile's left wave is off the zero-column torso path (a non-finite M in 30 / 31, a
    huge one in 32 / 33), so that wave runs the general fit while the block's other tile stays on the short one --
    tile 0 then tile 1."""
    ins, idx = _inputs()
    ref = _reference("shipped", True)
    st = ref["status"][idx.cpu().numpy()]
    assert st[128 * 30 + 5] == 1 and st[128 * 31 + 69] == 1 and st[128 * 32 + 9] == 0 and st[128 * 33 + 73] == 0
    assert st[128 * 30:128 * 34].sum() == 2
    B = LAT + 1
    _check(_solver("shipped", True), ref, tuple(t[:B] for t in ins), idx[:B], layout, True, f"mixed {layout}",
           rows=slice(128 * 30, 128 * 34))


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_raising_frame_alone_in_a_one_row_tile(gpu, layout):
    """The batch's last row is a frame the reference raises on (torso | left wrist | right wrist | all), alone in its
    tile, for each of the three ragged batches."""
    ins, idx = _inputs()
    pool = tuple(torch.from_numpy(a).cuda() for a in _pool())
    ref = _reference("shipped", True)
    S = _solver("shipped", True)
    for extra in EXTRAS:
        B = LAT + extra
        for kind in KINDS:
            s = SP[f"nan_{kind}"]
            assert ref["status"][s] == 1
            bi = idx[:B].clone()
            bi[B - 1] = s
            bins = tuple(t[:B].clone() for t in ins)
            for t, p in zip(bins, pool):
                t[B - 1] = p[s]
            _check(S, ref, bins, bi, layout, True, f"B={B} last row nan_{kind} {layout}", rows=slice(LAT - 128, B))

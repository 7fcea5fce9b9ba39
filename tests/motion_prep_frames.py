"""Hostile input for the motion-level prep of retarget/main.py (rescale_motion, quat_between_two_vecs, rebuild_vtrdyn) and
for the teleop ingest (a helper module: host numpy only, so the CPU tests, the GPU tests and tools/make_golden.py build
the same arrays).  _rng and placements are those of tests/kinematics_frames.py.

pair_batches(B) -> {name: (v1, v2)}: batches for quat_between_two_vecs.  The function returns the identity for the whole
batch when the largest norm of either side is <= 1e-6f, so the decision cases put ONE deciding row above a rest of zero
rows (or rows of 1e-7) on one side, the other side ordinary; pair_identity(name) says which branch the name promises.
decision_pair(B, side, length, row, rest) builds one such batch with the deciding row where the caller wants it.
motions(family, B) -> (B, 21, 3) raw VTRDyn positions from the 64-frame clip of tests/golden/motion_prep.npz, tiled and
jittered as tests/test_gpu_parity.py does; SCALE_NONFINITE states per scale_<s> family whether every rescaled frame is
non-finite or none is.  A bone of an exact length needs its parent end at the origin (x + 1e-7 rounds to x for a
joint half a metre out), so the families that set a length put the parent joint at 0.
rebuild_decision(B, joint, length, row, rest) is the rebuild's form of decision_pair: bone `joint` of a tame batch.
topologies(parents) -> {name: (parent table, local_t, motion (B, J, 3))} for the rescale, which takes any tree.
ingest_values() -> the body values about the 1e-8 flag threshold.

Everything is deterministic from the seeds."""
import os

import numpy as np

from kinematics_frames import _rng, placements

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
EPS = F32(1e-6)                                   # the batch-level threshold of quat_between_two_vecs
EPS_BELOW, EPS_ABOVE = np.nextafter(EPS, F32(0)), np.nextafter(EPS, F32(1))
# name -> (deciding length, the rest of the rows: 0 or 1e-7, the whole batch comes back as the identity)
DECISIONS = {"0": (F32(0), 0.0, True), "1e-45": (F32(1e-45), 0.0, True), "eps_below": (EPS_BELOW, 1e-7, True),
             "eps": (EPS, 1e-7, True), "eps_above": (EPS_ABOVE, 1e-7, False), "1e-5": (F32(1e-5), 1e-7, False)}
MIXED_ROWS = ("zero_v1", "zero_v2", "antiparallel", "antiparallel_ulp", "parallel_3x", "scale_1e-30", "scale_1e-23",
              "scale_1e-19", "scale_1e18", "scale_1e19", "scale_1e25", "signed_zero", "nan", "inf", "neg_inf")

VTRDYN_PARENTS = None                             # filled from rtg.assets on first use
KABSCH_POINTS = (1, 4, 7, 11, 13, 17)             # main.py:126-134: the fits of joints 0 and 10 read these and 0, 10
CHAIN_JOINTS, LEAF_JOINTS = (5, 14, 19, 2, 8), (3, 6, 12, 16, 20)
SCALES = (1e-38, 1e-30, 1e-22, 1e-20, 1e-18, 1e15, 1e19, 1e25, 1e37)
# every rescaled frame non-finite (True) or none (False).  A bone of the clip is 0.04 .. 0.6 m: scaled by 1e-22 or less
# the squared length of at least one bone per frame is below half the least subnormal (0.7e-45), the norm 0 and the
# quotient 0 / 0; by 1e-20 every squared length is above 1e-43 and by 1e-18 normal: a nonzero norm, a finite quotient.
# From 1e25 a squared length overflows, the norm and the scale are inf and d / inf = 0: every joint lands on the root.
SCALE_NONFINITE = {1e-38: True, 1e-30: True, 1e-22: True, 1e-20: False, 1e-18: False, 1e15: False, 1e19: False,
                   1e25: False, 1e37: False}
ZERO_BONE_JOINTS = (2, 15, 10)                    # under the Kabsch point 1, mid-chain, joint 10 under 9
TINY_BONE = 15                                    # tiny_bone_every_frame: the bone 14 -> 15
SINGLES = ("zero_bone_single", "nan_single", "inf_single", "subnormal_bone_single", "huge_single")
MOTION_FAMILIES = ("tame",) + tuple(f"scale_{s:g}" for s in SCALES) + \
    tuple(f"zero_bone_every_frame_{j}" for j in ZERO_BONE_JOINTS) + \
    tuple(f"tiny_bone_every_frame_{d}" for d in DECISIONS) + SINGLES + ("collapsed", "coplanar_torso", "mirrored")
B_GPU = (1, 63, 64, 65, 255, 256, 257, 513)       # one wave, one 256-thread block, ragged on both sides
DECIDING_ROWS = (0, 63, 64, 255, 256, 511, 512)   # of B = 513: first / last lane of a wave, other wave, other block, tail


def parents():
    global VTRDYN_PARENTS
    if VTRDYN_PARENTS is None:
        from rtg import assets
        VTRDYN_PARENTS = np.asarray(assets.parents("vtrdyn"), np.int64)
    return VTRDYN_PARENTS


def _unit_rows(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _ordinary(rng, n):
    return (_unit_rows(rng, n) * rng.uniform(0.1, 1.0, (n, 1))).astype(F32)


def _axis_row(length, k):
    """(.., length, ..) on component k % 3, negated for odd k // 3: its float32 norm is |length| exactly (sqrt(RN(x^2)) == |x|
    in binary floating point unless x^2 underflows: 1e-45 has the norm 0)."""
    r = np.zeros(3, F32)
    r[k % 3] = -length if (k // 3) % 2 else length
    return r


def _rest_rows(rng, n, rest):
    return (_unit_rows(rng, n) * rest).astype(F32) if rest else np.zeros((n, 3), F32)


def decision_pair(B, side, length, row, rest, seed=0):
    """(v1, v2) of B rows: side `side` (1 or 2) holds `rest` rows (0: zeros, else random rows of that length) and one
    row of the float32 norm `length` (a NaN or inf `length` puts that value in one component) at `row`; the other side is
    ordinary (0.1 .. 1)."""
    rng = _rng("pair", B, side, row, float(rest), seed)
    small = _rest_rows(rng, B, rest)
    small[row] = _axis_row(F32(length), row)
    other = _ordinary(rng, B)
    return (small, other) if side == 1 else (other, small)


def mixed_rows(B, seed=0, kinds=MIXED_ROWS):
    """B ordinary pairs with one row of each MIXED_ROWS kind (spread over the batch; for B below the number of kinds the
    first B kinds), and the row index of each kind.  kinds = (): the ordinary pairs alone."""
    rng = _rng("mixed", B, seed)
    v1, v2 = _ordinary(rng, B), _ordinary(rng, B)
    nk = len(MIXED_ROWS)
    at = {}
    for k, kind in enumerate(MIXED_ROWS[:B]):
        if kind not in kinds:
            continue
        r = k if B < 2 * nk else (k * B) // nk + (B // nk) // 2
        at[kind] = r
        if kind == "zero_v1":
            v1[r] = 0.0
        elif kind == "zero_v2":
            v2[r] = 0.0
        elif kind == "antiparallel":
            v2[r] = -v1[r]
        elif kind == "antiparallel_ulp":
            v2[r] = -v1[r]
            v2[r, k % 3] = np.nextafter(v2[r, k % 3], F32(0))
        elif kind == "parallel_3x":
            v2[r] = v1[r] * F32(3)
        elif kind.startswith("scale_"):
            s = float(kind[6:])
            v1[r], v2[r] = (v1[r].astype(np.float64) * s).astype(F32), (v2[r].astype(np.float64) * s).astype(F32)
        elif kind == "signed_zero":
            v1[r], v2[r] = (0.0, -0.0, 0.5), (-0.0, 0.25, -0.0)
        elif kind == "nan":
            v1[r, 1] = np.nan
        elif kind == "inf":
            v2[r, 2] = np.inf
        elif kind == "neg_inf":
            v1[r, 0] = -np.inf
    return v1, v2, at


def pair_batches(B=16, seed=0):
    """{name: (v1, v2)}: the six decision cases on either side (the deciding row in the middle of the batch), all-small
    batches with one NaN row and with one inf row on either side, and the mixed batch."""
    out = {}
    row = B // 2
    for side in (1, 2):
        for name, (length, rest, _) in DECISIONS.items():
            out[f"v{side}_{name}"] = decision_pair(B, side, length, row, rest, seed)
        out[f"v{side}_small_one_nan"] = decision_pair(B, side, np.nan, row, 1e-7, seed)
        out[f"v{side}_small_one_inf"] = decision_pair(B, side, np.inf, row, 1e-7, seed)
    out["mixed"] = mixed_rows(B, seed)[:2]
    return out


def pair_identity(name, B=16):
    """Whether the batch `name` of pair_batches(B) takes the identity branch (torch.max gives NaN for a NaN row, and NaN
    <= 1e-6 is false; an inf row is the maximum).  The mixed batch of one row is its zero_v1 row alone."""
    if name == "mixed":
        return B == 1
    if name.endswith(("one_nan", "one_inf")):
        return False
    return DECISIONS[name[3:]][2]


# ---------------------------------------------------------------------------------------------------- motions
_CLIP = []


def _clip():
    if not _CLIP:
        _CLIP.append(np.load(os.path.join(GOLDEN, "motion_prep.npz"))["raw"])
    return _CLIP[0]


def tame(B, seed=0):
    raw = _clip()
    rng = _rng("motion", B, seed)
    return (raw[rng.integers(0, len(raw), B)] * rng.uniform(0.7, 1.3, (B, 1, 1))
            + rng.normal(0, 0.02, (B, 21, 3))).astype(F32)


def single_frames(B):
    """The frames a *_single family touches: placements(B, (64, 256)) and, in a short batch, every third frame."""
    t = set(placements(B, tiles=(64, 256)))
    if B <= 32:
        t |= set(range(2, B - 2, 3))
    return sorted(t)


def single_joint(i):
    """The joint of the i-th touched frame: a Kabsch point, joint 0, joint 10, a chain joint, a leaf in turn."""
    k = i // 5
    return (KABSCH_POINTS[k % 6], 0, 10, CHAIN_JOINTS[k % 5], LEAF_JOINTS[k % 5])[i % 5]


def set_single(m, kind, t, j):
    """One hostile element of the motion m (B, 21, 3) at frame t, joint j, in place."""
    p = int(parents()[j])
    c = (t + j) % 3
    if kind == "nan_single":
        m[t, j, c] = np.nan
    elif kind == "inf_single":
        m[t, j, c] = np.inf if (t + j) % 2 == 0 else -np.inf
    elif kind == "huge_single":
        m[t, j, c] = 1e25
    elif kind == "zero_bone_single":
        if j == 0:
            m[t, [1, 4, 7]] = m[t, 0]              # the root has no bone: its three children on it
        else:
            m[t, j] = m[t, p]
    elif kind == "subnormal_bone_single":          # the parent end at the origin, the bone (1e-30, 0, 0): |d|^2 underflows
        if j == 0:
            m[t, 0], m[t, 1] = 0.0, (1e-30, 0.0, 0.0)
        else:
            m[t, p], m[t, j] = 0.0, (1e-30, 0.0, 0.0)
    else:
        raise KeyError(kind)


def rebuild_decision(B, joint, length, row, rest, seed=0):
    """A tame batch whose bone parent(joint) -> joint is `rest` long in every frame (0: zero) but `row`, where its float32
    length is `length` exactly (NaN / inf: that value in one component); the parent joint sits at the origin."""
    m = tame(B, seed)
    rng = _rng("bone", B, joint, row, float(rest), seed)
    m[:, int(parents()[joint])] = 0.0
    m[:, joint] = _rest_rows(rng, B, rest)
    m[row, joint] = _axis_row(F32(length), row)
    return m


def motions(family, B, seed=0):
    if family not in MOTION_FAMILIES:
        raise KeyError(family)
    m = tame(B, seed)
    par = parents()
    if family.startswith("scale_"):
        with np.errstate(all="ignore"):
            m = (m.astype(np.float64) * float(family[6:])).astype(F32)
    elif family.startswith("zero_bone_every_frame_"):
        j = int(family.rsplit("_", 1)[1])
        m[:, j] = m[:, par[j]]
    elif family.startswith("tiny_bone_every_frame_"):
        length, rest, _ = DECISIONS[family[len("tiny_bone_every_frame_"):]]
        m = rebuild_decision(B, TINY_BONE, length, B // 2, rest, seed)
    elif family in SINGLES:
        for i, t in enumerate(single_frames(B)):
            set_single(m, family, t, single_joint(i))
    elif family == "collapsed":
        m[:] = m[:, :1]
    elif family == "coplanar_torso":               # 1, 4, 7 on one line through joint 0: a rank-1 Kabsch matrix
        u = _unit_rows(_rng("coplanar", B, seed), B).astype(F32)
        for k, a in ((1, 0.11), (4, -0.23), (7, 0.35)):
            m[:, k] = m[:, 0] + F32(a) * u
    elif family == "mirrored":
        m[..., 0] = -m[..., 0]
    return np.ascontiguousarray(m)


def svd_input_has_nan(m, zl):
    """Whether a Kabsch matrix M^T Z of rebuild_vtrdyn(m) (joints 0 and 10, main.py:126-134) holds a NaN: the batched
    torch.linalg.svd raises for the whole batch then.  An inf point makes one by inf - inf or inf * 0."""
    m, zl = np.asarray(m, F32), np.asarray(zl, F32)
    with np.errstate(all="ignore"):
        A = [np.einsum("bji,jk->bik", m[:, pts] - m[:, [c]], zl[pts]) for c, pts in ((0, [4, 1, 7]), (10, [17, 13, 11]))]
    return bool(np.isnan(A).any())


def fixture_pairs():
    """The pair batches tests/golden/motion_prep_adversarial.npz records: 16 rows each, the mixed batch 24."""
    out = pair_batches(16)
    out["mixed"] = mixed_rows(24)[:2]
    return out


def fixture_motion(family):
    """The motion the fixture records for a family: 16 frames, 24 for the *_single families (11 touched frames)."""
    return motions(family, 24 if family in SINGLES else 16)


# ---------------------------------------------------------------------------------------------------- topologies
def topologies(tree_parents, local_t, B=8, seed=0):
    """{name: (parents, local_t, motion (B, J, 3))}: tree_parents / local_t map "vtrdyn" and "vtrdyn_full" to their tables
    (the zero poses); then a one-joint tree and a 5-chain whose local_t has a zero row, a 1e-30 row, a 1e25 row and a NaN
    row (|zl| = 0, subnormal -- its square underflows --, inf and NaN as the divisor of the scale)."""
    out = {}
    for name in ("vtrdyn", "vtrdyn_full"):
        p = np.asarray(tree_parents[name], np.int32)
        out[name] = (p, np.ascontiguousarray(local_t[name], F32),
                     _rng("topo", name, B, seed).normal(0, 0.4, (B, len(p), 3)).astype(F32))
    out["one"] = (np.array([-1], np.int32), np.zeros((1, 3), F32), _rng("topo", 1, B, seed).normal(size=(B, 1, 3)).astype(F32))
    lt = np.array([[0, 0, 0], [0, 0, 0], [1e-30, 0, 0], [0, 1e25, 0], [0.1, np.nan, 0.2]], F32)
    out["chain5"] = (np.arange(-1, 4, dtype=np.int32), lt, _rng("topo", 5, B, seed).normal(0, 0.4, (B, 5, 3)).astype(F32))
    return out


# ---------------------------------------------------------------------------------------------------- ingest
ATOL = F32(1e-8)                                   # np.allclose(x, 0): |x| <= 1e-8 (rtol times 0 adds nothing)


def ingest_values():
    """The body values about the "frame carries data" flag of the teleop loop (not np.allclose(body_pos, 0))."""
    up, down = np.nextafter(ATOL, F32(1)), np.nextafter(ATOL, F32(0))
    return [F32(v) for v in (0.0, -0.0, 1e-45, ATOL, down, up, -ATOL, -up, 1e-7, np.nan, np.inf, -np.inf)]


def carries_data(x):
    """The kernel's predicate restated: !(|x| <= 1e-8f) over the values of a frame."""
    with np.errstate(all="ignore"):
        return bool((~(np.abs(np.asarray(x, F32)) <= ATOL)).any())

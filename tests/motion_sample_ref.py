"""Test-side reference of the motion sampler (rtg.h rtg_motion_sample_f32) composed from oracle primitives only, and
the builders of its hostile input.  Not a test module.

sample(lib, clip, time, ...) restates the index rule in numpy float64, gathers the two frames, applies
``oracle.quat_slerp`` (then ``oracle.quat_normalize``), blends the root translation and the vector rows with every one
of the four float32 operations computed in float64 and rounded to float32 (the correctly rounded float32 operation for
+, - and x, whatever numpy was compiled with) and runs ``oracle.fk`` / ``oracle.state_fk`` for the global outputs.  An
invalid query (clip id outside 0..C-1) is the quiet NaN 0x7FC00000 everywhere.

Library: a dict with rot (F_total, J, 4), root_t (F_total, 3), vec (F_total, K, 3) | None, start (C) int64, len (C)
int32, fps (C) float32.  Quaternions are (x, y, z, w) rows; everything is deterministic from the seeds."""
import numpy as np

import oracle as orc
from kinematics_frames import ROT_FAMILIES, rot_sequence

QNAN = np.uint32(0x7FC00000)
LIB_LENGTHS = (1, 2, 3, 17, 130)
LIB_FPS = (30.0, 120.0, 32.0, 1.0, 59.94)


def bits(a):
    """float32 bits with every NaN reading alike (NaN sign / payload from arithmetic differs between hosts); the sign of
    zero is kept."""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), QNAN, a.view(np.uint32))


def f32(x):
    with np.errstate(all="ignore"):
        return np.asarray(x, np.float64).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the index rule
def index_rule(clip, time, length, fps):
    """Steps 1-3 of the contract, numpy float64 -> (valid, i0, i1, b float32), each (N).  Invalid queries get i0 = i1 =
    0, b = 0."""
    clip = np.asarray(clip, np.int64)
    C = len(length)
    valid = (clip >= 0) & (clip < C)
    c = np.where(valid, clip, 0)
    L = np.asarray(length, np.int64)[c]
    with np.errstate(all="ignore"):
        p = np.asarray(time, np.float32).astype(np.float64) * np.asarray(fps, np.float32).astype(np.float64)[c]
    p = np.where(p > 0, p, 0.0)                       # NaN, -0 and negatives
    end = p >= (L - 1)
    with np.errstate(all="ignore"):
        i0 = np.where(end, L - 1, np.trunc(np.where(end, 0.0, p))).astype(np.int64)
    i1 = np.where(end, i0, i0 + 1)
    b = np.where(end, 0.0, p - i0).astype(np.float32)
    z = np.zeros_like(i0)
    return valid, np.where(valid, i0, z), np.where(valid, i1, z), np.where(valid, b, np.float32(0))


def blend(a, c, b):
    """torch's (1 - b) * a + b * c in float32: four roundings, no FMA.  b broadcasts over the trailing axes."""
    a64, c64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(c, np.float32).astype(np.float64)
    b64 = np.asarray(b, np.float32).astype(np.float64).reshape((-1,) + (1,) * (a64.ndim - 1))
    with np.errstate(all="ignore"):
        om = f32(1.0 - b64).astype(np.float64)
        t1 = f32(om * a64).astype(np.float64)
        t2 = f32(b64 * c64).astype(np.float64)
        return f32(t1 + t2)


def sample(lib, clip, time, normalize=False, tree=None, state=False):
    """-> dict(local_rot, root_t, vec | None, g_rot | None, g_pos | None, valid, row0, row1, b).  tree = (parents,
    local_t, tree_quat) asks for the global outputs (state: oracle.state_fk, else oracle.fk)."""
    rot, root_t, vec = lib["rot"], lib["root_t"], lib.get("vec")
    N, J = len(clip), rot.shape[1]
    valid, i0, i1, b = index_rule(clip, time, lib["len"], lib["fps"])
    st = np.asarray(lib["start"], np.int64)[np.where(valid, np.asarray(clip, np.int64), 0)]
    r0, r1 = np.where(valid, st + i0, 0), np.where(valid, st + i1, 0)
    assert N == 0 or (r0.min() >= 0 and r1.max() < len(rot))
    nan = np.float32(np.nan)
    out = {"valid": valid, "row0": r0, "row1": r1, "b": b}
    q = orc.quat_slerp(rot[r0].reshape(-1, 4), rot[r1].reshape(-1, 4), np.repeat(b, J)) if N else np.zeros((0, 4), np.float32)
    if normalize and N:
        q = orc.quat_normalize(q)
    q = q.reshape(N, J, 4)
    q[~valid] = nan
    rt = blend(root_t[r0], root_t[r1], b)
    rt[~valid] = nan
    out["local_rot"], out["root_t"] = q, rt
    out["vec"] = None
    if vec is not None:
        v = blend(vec[r0], vec[r1], b)
        v[~valid] = nan
        out["vec"] = v
    out["g_rot"] = out["g_pos"] = None
    if tree is not None:
        parents, local_t, tq = tree
        if N == 0:
            gr, gp = np.zeros((0, J, 4), np.float32), np.zeros((0, J, 3), np.float32)
        elif state:
            gr, gp = orc.state_fk(parents, tq, local_t, q, rt)
        else:
            gr, gp = orc.fk(parents, local_t, q, rt)
        gr[~valid] = nan
        gp[~valid] = nan
        out["g_rot"], out["g_pos"] = gr, gp
    return out


# ------------------------------------------------------------------------------------------------ input builders
def random_tree(J, seed=0):
    """(parents int32, local_t (J, 3), tree_quat (J, 4)): a random tree of J joints with non-trivial tree quaternions."""
    rng = np.random.default_rng(1000 + 7 * J + seed)
    parents = np.array([-1] + [int(rng.integers(max(0, j - 6), j)) for j in range(1, J)], np.int32)
    lt = rng.normal(0, 0.2, (J, 3)).astype(np.float32)
    tq = rng.normal(size=(J, 4))
    tq = (tq / np.linalg.norm(tq, axis=1, keepdims=True)).astype(np.float32)
    return parents, lt, tq


def make_library(J, family="smooth", lengths=LIB_LENGTHS, fps=LIB_FPS, K=None, seed=0, only_joint=None):
    """Clips of `lengths` frames at `fps`, rotations of kinematics_frames.rot_sequence(family) (on every joint, or on
    `only_joint` of an otherwise smooth clip), random root translations and vector rows."""
    rng = np.random.default_rng(5000 + 31 * J + seed)
    rots = []
    for c, L in enumerate(lengths):
        r = rot_sequence(family, L, J, seed + c)
        if only_joint is not None:
            base = rot_sequence("smooth", L, J, seed + c)
            base[:, only_joint % J] = r[:, only_joint % J]
            r = base
        rots.append(r)
    Ft = int(sum(lengths))
    lib = {"rot": np.ascontiguousarray(np.concatenate(rots), np.float32),
           "root_t": rng.normal(0, 0.5, (Ft, 3)).astype(np.float32),
           "vec": None if not K else rng.normal(0, 1.0, (Ft, K, 3)).astype(np.float32),
           "start": np.concatenate([[0], np.cumsum(lengths[:-1])]).astype(np.int64),
           "len": np.asarray(lengths, np.int32), "fps": np.asarray(fps, np.float32)}
    return lib


# slerp's two thresholds (transform3d.py:152-174): with q0 the identity and q1 = (x, 0, 0, c), the float32 cosine of
# the half angle is c exactly, and sin = sqrt(1 - RN(c c)).  A float32 c in [1/2, 1) is 1 - m 2^-24, and RN(c c) =
# 1 - 2 m 2^-24 for small m, so sin = sqrt(2 m) 2^-12: 0.001f lies between m = 8 (sin = 2^-10 = 0.0009765625) and
# m = 9 (0.0010358), and NO float32 cosine gives sin == 0.001f exactly -- the pairs sit on its two nearest reachable
# neighbours.  name -> (c, x, the branch slerp takes)
_U = 2.0 ** -24
THRESHOLD_CASES = {
    "sin_below": (1 - 8 * _U, np.sqrt(1 - (1 - 8 * _U) ** 2), "midpoint"),     # the largest reachable sin below 0.001f
    "sin_above": (1 - 9 * _U, np.sqrt(1 - (1 - 9 * _U) ** 2), "slerp"),        # the smallest reachable sin above it
    "sin_far_above": (1 - 64 * _U, np.sqrt(1 - (1 - 64 * _U) ** 2), "slerp"),
    "cos_one": (1.0, 0.25, "q0"),                                             # cos == 1.0f from a non-unit row
    "cos_below_one": (1 - _U, np.sqrt(1 - (1 - _U) ** 2), "midpoint"),        # the float32 neighbour below 1
    "cos_above_one": (1.5, 0.5, "q0"),                                        # above 1 from a non-unit row
    "cos_minus_one": (-1.0, 0.25, "q0"),                                      # the flip, then cos == 1
    "sin_above_flipped": (-(1 - 9 * _U), np.sqrt(1 - (1 - 9 * _U) ** 2), "slerp"),
}


def threshold_pairs():
    """-> (names, q0 (n, 4), q1 (n, 4)) float32."""
    names = list(THRESHOLD_CASES)
    q0 = np.tile(np.array([0, 0, 0, 1], np.float32), (len(names), 1))
    q1 = np.array([[THRESHOLD_CASES[n][1], 0.0, 0.0, THRESHOLD_CASES[n][0]] for n in names]).astype(np.float32)
    return names, q0, q1


def threshold_library(J):
    """One clip per threshold case, two frames each (fps 1): joint j of frame 0 is the identity, of frame 1 the case's
    q1, so a query at time b blends the pair with factor b."""
    names, q0, q1 = threshold_pairs()
    rot = np.stack([np.repeat(q[:, None], J, axis=1) for q in (q0, q1)], axis=1).reshape(-1, J, 4)
    n = len(names)
    rng = np.random.default_rng(9)
    return {"rot": np.ascontiguousarray(rot, np.float32), "root_t": rng.normal(0, 0.5, (2 * n, 3)).astype(np.float32),
            "vec": None, "start": (2 * np.arange(n)).astype(np.int64), "len": np.full(n, 2, np.int32),
            "fps": np.ones(n, np.float32)}, names


def find_b_one(fps, L):
    """Host search for times whose blend factor rounds up to 1.0f on a clip of L frames at fps: the float32 times
    around k / fps with frac(time fps) >= 1 - 2^-25.  -> float32 array (possibly empty)."""
    f = float(np.float32(fps))
    hits = []
    for k in range(1, L - 1 + 1):
        t = np.float32(k / f)
        for _ in range(3):
            p = float(t) * f
            if 0 < p < L - 1 and np.float32(p - np.trunc(p)) == np.float32(1.0):
                hits.append(t)
            t = np.nextafter(t, np.float32(-np.inf))
    return np.array(hits, np.float32)


def time_family(L, fps):
    """Every time family for a clip of L frames at fps, one float32 array: the frame instants and one ulp either side,
    a point inside every consecutive pair, 0, -0.0, negative, subnormal, the last frame's instant, past the end, +-inf,
    NaN, and the times whose b rounds up to 1.0f where the host search finds some."""
    f = float(np.float32(fps))
    inst = (np.arange(L) / f).astype(np.float32)
    inf = np.float32(np.inf)
    mid = ((np.arange(max(L - 1, 1)) + 0.37) / f).astype(np.float32)
    edge = np.array([0.0, -0.0, -1.0, -1e-30, 1e-45, -1e-45, (L - 1) / f, L / f, (L + 100.5) / f, 3e38, np.inf, -np.inf,
                     np.nan], np.float32)
    return np.concatenate([inst, np.nextafter(inst, inf), np.nextafter(inst, -inf), mid, edge, find_b_one(fps, L)])


def library_queries(lib):
    """Every time family on every clip of the library -> (clip int32, time float32)."""
    cs, ts = [], []
    for c, (L, f) in enumerate(zip(lib["len"], lib["fps"])):
        t = time_family(int(L), float(f))
        cs.append(np.full(len(t), c, np.int32))
        ts.append(t)
    return np.concatenate(cs), np.concatenate(ts)


FIXTURE_J = 4


def fixture_cases():
    """family -> (library, clip (8), time (8)) of tests/golden/motion_sample.npz (tools/make_golden.py motion_sample
    runs the reference on them): every rotation family of kinematics_frames on a 4-joint library, the slerp threshold
    pairs, the time families (taken evenly from every clip) and invalid clip ids."""
    J, cases = FIXTURE_J, {}
    for fam in ROT_FAMILIES:
        lib = make_library(J, fam, K=2, seed=3)
        c, t = library_queries(lib)
        between = np.flatnonzero((c >= 3) & np.isfinite(t) & (t > 0))     # the 17- and 130-frame clips
        pick = between[np.linspace(0, len(between) - 1, 8).astype(int)]
        cases[fam] = (lib, c[pick], t[pick])
    lib, names = threshold_library(J)
    cases["thresholds"] = (lib, np.arange(8, dtype=np.int32) % len(names), np.full(8, 0.25, np.float32))
    lib = make_library(J, "smooth", K=2, seed=4)
    c, t = library_queries(lib)
    for k in range(4):                                                   # the time families, 8 queries at a time
        pick = np.arange(k, len(c), max(1, len(c) // 8))[:8]
        cases[f"times_{k}"] = (lib, c[pick], t[pick])
    cases["invalid"] = (lib, np.array([-1, 5, 0, 4, -2**31, 2**31 - 1, 6, 2], np.int32),
                        np.array([0.0, 0.1, 0.01, 1.0, 0.5, 0.5, np.nan, 0.03], np.float32))
    return cases


__all__ = ["ROT_FAMILIES", "sample", "index_rule", "blend", "bits", "make_library", "threshold_pairs",
           "threshold_library", "time_family", "library_queries", "random_tree", "find_b_one"]

"""Hostile input for the motion-velocity kernels and the FK family (a helper module: host numpy only, so the CPU
tests, the GPU tests and tools/make_golden.py build the same arrays).  The quaternion helpers, W_EDGES, SCALES_Q and the
18 per-row quaternion family names are those of tests/other_solver_frames.py.

rot_sequence(family, L, J, seed) -> (L, J, 4): rotation sequences for the angular velocity.  What the kernel sees is the
pair (t, t + 1), so a family chooses the relative rotation d_t and sets r[t + 1] = d_t * r[t] in float64, the whole
sequence rounded to float32 once; the families that need an exact relative rotation (a w exactly on an edge, an
imaginary part of 1e-20) keep some joints on single-axis rows about the identity, where the float32 product is exact.
pos_sequence(family, L, J, seed) -> (L, J, 3): position sequences for the linear velocity.
placements(L) -> the frames a single bad element is put at: both ends and both sides of every 16 / 32 / 64-frame tile
boundary.  fk_rotations(J, per_family, seed) -> (18 * per_family, J, 4): per-frame rotations for the FK family, each
family on every row of a frame (the first half of its frames) or on a random tenth of the rows.

Quaternions are (x, y, z, w) rows; everything is deterministic from the seeds."""
import zlib

import numpy as np

from other_solver_frames import (SCALES_Q, W_EDGES, _QUAT_FAMILIES, _f32, _unit3, axis_quat, gimbal_quat,
                                 near_unit_factor, qmul, rand_unit, w_edge_quat)

ROT_FAMILIES = ("static", "antipodal", "half_turn", "tiny_step", "w_edges", "near_unit", "nonunit") + \
    tuple(f"scale_{s:g}" for s in SCALES_Q) + ("zero_row", "nan", "inf", "zero_row_single", "nan_single", "inf_single",
                                               "smooth")
POS_FAMILIES = ("static", "ramp", "subnormal", "huge", "cancel", "nan", "inf", "random")
FK_FAMILIES = tuple(f[0] for f in _QUAT_FAMILIES)
TILES = (16, 32, 64)
TINY_ANGLES = (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9)
# imaginary parts of an exact relative rotation (x, 0, 0, 1): |xyz|^2 normal, subnormal (1e-20 .. 1e-22) and underflowing
# to zero, each below the 1e-9 clamp of the axis normalisation, and values about the clamp
TINY_PARTS = (1e-2, 1e-5, 2e-9, 1e-9, 5e-10, 1e-12, 1e-19, 1e-20, 3e-22, 1e-23, 1e-30, 1e-40, 1e-45, 0.0)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def qmul_rows(a, b):
    """other_solver_frames.qmul over the last axis of (..., 4) arrays."""
    return np.moveaxis(qmul(np.moveaxis(a, -1, 0), np.moveaxis(b, -1, 0)), 0, -1)


def placements(L, tiles=TILES):
    """Frames 0, 1, L - 2, L - 1 and k T - 1, k T for every tile length T: sorted, within [0, L)."""
    t = {0, 1, L - 2, L - 1}
    for T in tiles:
        for k in range(T, L, T):
            t |= {k - 1, k}
    return sorted(x for x in t if 0 <= x < L)


def smooth(L, J, rng):
    """tools/make_golden.py gen_motion's rotations: cumulative small axis-angle steps per joint (float64, unit)."""
    steps = rng.normal(0, 0.05, (L, J, 3)).cumsum(0)
    ang = np.linalg.norm(steps, axis=-1, keepdims=True)
    return np.concatenate([steps / np.maximum(ang, 1e-12) * np.sin(ang / 2), np.cos(ang / 2)], -1)


def _rand_units(rng, n):
    return np.stack([rand_unit(rng) for _ in range(n)])


def _small_steps(rng, J, angles):
    ax = rng.normal(size=(J, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    a = np.asarray(angles, np.float64).reshape(-1, 1)
    return np.concatenate([ax * np.sin(a / 2), np.cos(a / 2) * np.ones((J, 1))], axis=1)


def set_single(x, kind, t, j, rng=None):
    """One bad element of the sequence x (L, J, 3 | 4) float32 at frame t, joint j, in place: 'nan' / 'inf' one component,
    'zero_row' the whole row."""
    c = (t + j) % x.shape[-1]
    if kind == "zero_row":
        x[t, j] = 0.0
    elif kind == "nan":
        x[t, j, c] = np.nan
    elif kind == "inf":
        x[t, j, c] = np.inf if (t + j) % 2 == 0 else -np.inf
    else:
        raise KeyError(kind)


def rot_sequence(family, L, J, seed=0):
    rng = _rng("rot", family, L, J, seed)
    if family not in ROT_FAMILIES:
        raise KeyError(family)
    if family in ("static", "antipodal", "half_turn", "tiny_step", "w_edges"):
        r = np.empty((L, J, 4))
        r[0] = _rand_units(rng, J)
        exact = np.arange(J) % 2 == 1          # joints kept on single-axis rows about the identity
        if family == "static":
            zs = np.array([[0.0, -0.0, 0.0, 1.0], [-0.0, 0.0, 1.0, -0.0], [1.0, 0.0, -0.0, 0.0], [-0.0, -0.0, -0.0, -1.0]])
            r[0, exact] = zs[np.arange(int(exact.sum())) % 4]
        elif family != "antipodal":
            r[0, exact] = (0.0, 0.0, 0.0, 1.0)
        for t in range(L - 1):
            if family == "static":              # runs of 1 .. 9 identical frames, a small step between runs
                r[t + 1] = r[t]
                move = rng.random(J) < 0.2
                if move.any():
                    r[t + 1, move] = qmul_rows(_small_steps(rng, int(move.sum()), rng.uniform(0.01, 0.3, int(move.sum()))),
                                               r[t, move])
            elif family == "antipodal":
                d = _small_steps(rng, J, rng.choice([0.0, 1e-3, 0.05], J))
                still = rng.random(J) < 0.3
                r[t + 1] = np.where(still[:, None], r[t], qmul_rows(d, r[t]))
                r[t + 1] *= np.where(rng.random(J) < 0.6, -1.0, 1.0)[:, None]
            elif family == "half_turn":
                d = np.stack([np.append(_unit3(rng), w) for w in rng.choice([0.0, -0.0, 1e-9, -1e-9, 3e-8, -3e-8], J)])
                r[t + 1] = qmul_rows(d, r[t])
                for j in np.flatnonzero(exact):   # half turns about one axis: the product's w is +-0 exactly
                    e = axis_quat((t + j) % 3, np.pi)
                    e[3] = (0.0, -0.0)[(t + j // 2) % 2]
                    r[t + 1, j] = qmul(e, r[t, j])
            elif family == "tiny_step":
                r[t + 1] = qmul_rows(_small_steps(rng, J, [TINY_ANGLES[(t + j) % len(TINY_ANGLES)] for j in range(J)]), r[t])
                for j in np.flatnonzero(exact):
                    # the identity and, in turn, (x e_k, 1) -- the product is (+-x e_k, 1): no angle, an axis below the
                    # clamp -- or an ordinary rotation about e_k with x on the next axis: a velocity component of ~x
                    r[t + 1, j] = (0.0, 0.0, 0.0, 1.0)
                    m, k = t // 2 + j // 2, (j // 2) % 3
                    x = TINY_PARTS[m % len(TINY_PARTS)] * (1, -1)[(t // 2) % 2]
                    if t % 4 == 0:
                        r[t + 1, j, k] = x
                    elif t % 4 == 2:
                        r[t + 1, j] = axis_quat(k, 0.1 + 0.2 * (m % 7))
                        r[t + 1, j, (k + 1) % 3] = x
            else:                                 # w_edges
                r[t + 1] = qmul_rows(np.stack([w_edge_quat(rng, t * J + j) for j in range(J)]), r[t])
                for j in np.flatnonzero(exact):   # the identity and an edge rotation in turn: the product's w is the edge
                    r[t + 1, j] = w_edge_quat(rng, t // 2 + j // 2) if t % 2 == 0 else (0.0, 0.0, 0.0, 1.0)
        return np.ascontiguousarray(_f32(r))
    r = smooth(L, J, rng)
    if family == "near_unit":
        r = r * near_unit_factor(rng.integers(-10, 11, (L, J, 1)).astype(np.float64))
    elif family == "nonunit":
        r = r * rng.uniform(0.5, 2.0, (L, J, 1))
    elif family.startswith("scale_"):
        r = r * float(family[6:])
    r = np.ascontiguousarray(_f32(r))
    if family == "zero_row":
        r[rng.random((L, J)) < 0.1] = 0.0
    elif family == "nan":
        r[rng.random((L, J, 4)) < 0.1] = np.nan
    elif family == "inf":
        m = rng.random((L, J, 4)) < 0.1
        r[m] = rng.choice([np.inf, -np.inf], int(m.sum()))
    elif family.endswith("_single"):
        for i, t in enumerate(placements(L)):
            set_single(r, family[:-7], t, (3 * i + 1) % J)
    return r


def pos_sequence(family, L, J, seed=0):
    rng = _rng("pos", family, L, J, seed)
    if family == "static":
        p0 = rng.normal(size=(J, 3))
        z = rng.random((J, 3))
        p0[z < 0.15] = 0.0
        p0[z > 0.85] = -0.0
        p = np.repeat(p0[None], L, axis=0)
        for t in range(1, L):                     # runs of identical frames, a step between runs
            move = rng.random(J) < 0.1
            p[t:, move] += rng.normal(0, 0.05, (int(move.sum()), 3))
    elif family == "ramp":                        # exact in float32: multiples of 1 / 64 below 2^10
        p = rng.integers(-256, 257, (1, J, 3)) / 64.0 + np.arange(L)[:, None, None] * rng.integers(-32, 33, (1, J, 3)) / 64.0
    elif family == "subnormal":
        p = rng.normal(size=(L, J, 3)) * 10.0 ** -rng.uniform(40, 45, (L, J, 3))
    elif family == "huge":
        p = rng.choice([3e38, -3e38, 1e38, 1.0], (L, J, 3))
    elif family == "cancel":
        # steps of ~1e-3 on 1e6 (below the float32 spacing there: runs of equal values and one-ulp jumps) and, on the
        # odd joints, on 1e3 (differences of a few ulps)
        base = np.where(np.arange(J) % 2 == 0, 1e6, 1e3)[None, :, None]
        p = base + 1e-3 * np.arange(L)[:, None, None] * rng.uniform(0.5, 2.0, (1, J, 3)) + rng.normal(0, 1e-4, (L, J, 3))
    elif family in ("nan", "inf", "random"):
        p = rng.normal(size=(L, J, 3))
    else:
        raise KeyError(family)
    p = np.ascontiguousarray(_f32(p))
    if family in ("nan", "inf"):
        for i, t in enumerate(placements(L)):
            set_single(p, family, t, (3 * i + 1) % J)
    return p


def _fk_row(fam, rng, j):
    q = rand_unit(rng)
    if fam == "unit":
        return q
    if fam == "nonunit":
        return q * rng.uniform(0.5, 2.0)
    if fam == "near_unit":
        return q * near_unit_factor(int(rng.integers(-40, 41)))
    if fam == "negated":
        return -q
    if fam == "identity":
        return np.array([0.0, 0.0, 0.0, 1.0])
    if fam == "half_turn":
        return axis_quat(j % 3, np.pi) if j % 4 != 3 else np.append(_unit3(rng), 0.0)
    if fam == "gimbal":
        return gimbal_quat(("XYZ", "YXZ", "ZYX")[j % 3], rng, j)
    if fam == "w_table_edges":
        return w_edge_quat(rng, j)
    if fam.startswith("scale_"):
        return q * float(fam[6:])
    if fam == "zero_row":
        return np.zeros(4)
    if fam in ("nan", "inf", "signed_zero"):
        q[int(rng.integers(4))] = {"nan": np.nan, "inf": rng.choice([np.inf, -np.inf]),
                                   "signed_zero": rng.choice([0.0, -0.0])}[fam]
        return q
    raise KeyError(fam)


def fk_rotations(J, per_family, seed=0):
    """(rot (18 * per_family, J, 4), root_t (.., 3), family index per frame).  Frame i of a family: the family on every
    row (i < per_family / 2) or on a random tenth of the rows, at least one, of a frame of unit rows.
    relative_identity: every chosen row is the same rotation, so a child's rotation relative to its parent is the
    identity up to rounding."""
    rng = _rng("fk", J, per_family, seed)
    n = len(FK_FAMILIES) * per_family
    rot = np.empty((n, J, 4))
    for k, fam in enumerate(FK_FAMILIES):
        for i in range(per_family):
            f = rot[k * per_family + i]
            f[:] = _rand_units(rng, J)
            rows = np.arange(J) if 2 * i < per_family else np.flatnonzero(rng.random(J) < 0.1)
            if len(rows) == 0:
                rows = np.array([int(rng.integers(J))])
            if fam == "relative_identity":
                f[rows] = rand_unit(rng)
            else:
                for j in rows:
                    f[j] = _fk_row(fam, rng, int(j) + i)
    root = rng.normal(0, 0.3, (n, 3))
    return np.ascontiguousarray(_f32(rot)), np.ascontiguousarray(_f32(root)), np.repeat(np.arange(len(FK_FAMILIES)), per_family)


# ---- quotients that are exact ties between two subnormal float32 values
# a / n with n = N 2^e (N odd, e >= 1) and a = N (2 j + 1) 2^(e - 150) is (2 j + 1) 2^-150 exactly: IEEE division rounds
# the tie to even, while a product by a rounded 1 / n lands beside the tie and rounds by the reciprocal's error.
def midpoint_dividends(n, count):
    """count float32 values a_j, j = 0 .. count - 1, with a_j / n == (2 j + 1) 2^-150 exactly (n an even integer with an
    odd factor).  The product by RN(1 / n) is off the tie by the reciprocal's relative error e, |e| <= 2^-53, and that
    survives the product's own rounding to float64 only if significand(2 j + 1) * |e| 2^53 > 1: for n = 10 (|e| 2^53 =
    0.5) never, for TIE_DIVISORS (0.93 .. 0.96) for about 45 % of the ties."""
    n = float(np.float32(n))
    a = np.array([n * (2 * j + 1) * 2.0 ** -150 for j in range(count)])
    assert (a.astype(np.float32).astype(np.float64) == a).all(), "n needs an even float32 value with an odd factor"
    return a.astype(np.float32)


def shortcut_misrounds(a, n):
    """Per dividend: whether float32(float64(a) * RN(1 / float64(n))) differs from the IEEE float32 quotient a / n."""
    a = np.asarray(a, np.float32)
    with np.errstate(all="ignore"):
        short = (a.astype(np.float64) * (1.0 / np.float64(np.float32(n)))).astype(np.float32)
        return short.view(np.uint32) != (a / np.float32(n)).view(np.uint32)


def midpoint_ramp(L, J, dt):
    """Positions (L, J, 3) whose every gradient, one-sided ones included, is a midpoint dividend of dt: channel c climbs
    by a_c per frame for 8 frames and falls back (there the gradient is -3 a_c: an odd multiple again), +- in turn."""
    a = midpoint_dividends(dt, 3 * J).astype(np.float64) * np.where(np.arange(3 * J) % 2, -1.0, 1.0)
    p = ((np.arange(L) % 8)[:, None] * a[None]).reshape(L, J, 3)
    assert (p.astype(np.float32).astype(np.float64) == p).all()
    return np.ascontiguousarray(p.astype(np.float32))


def tie_frame_times(raw_dt1, count):
    """Frame times dt = |a| 2^150 of `count` distinct raw velocities a computed with dt = 1 (0 < |a| < 2^-24, spread over
    their range): a / dt is 2^-150 exactly, the tie between 0 and the least subnormal."""
    a = np.abs(np.asarray(raw_dt1, np.float32).ravel())
    a = np.unique(a[(a > 0) & (a < np.float32(2.0 ** -24))])
    pick = a[np.linspace(0, len(a) - 1, min(count, len(a))).astype(int)]
    return [float(np.float32(float(x) * 2.0 ** 150)) for x in pick]


# even integers n below 4096 (n^2 is a float32) whose RN(1 / n) has a relative error of 0.89 .. 0.96 of 2^-53
TIE_DIVISORS = (246.0, 1006.0, 3994.0, 234.0, 958.0, 3846.0, 1910.0, 1990.0)
MIDPOINT_NORMS = TIE_DIVISORS
# RN(float32(pi) * 7 k 2^-127) / ANGULAR_TIE_DT is a tie for most odd k (float32(pi) = 3 * 5 * 878453 * 2^-22 and
# 127488 = 249 * 2^9, found by a host search over the divisors of the product's significand)
ANGULAR_TIE_DT = 127488.0


def angular_tie_sequence(L, J):
    """(L, J, 4): the identity and, in turn, a half turn (x, 1, 0, 0) (its axes rotated with the joint) with
    x = 7 (2 j + 1) 2^-127: the product is the row itself, its angle float32(pi), its axis (x, 1, 0), so the raw
    velocity before the division is RN(x pi) exactly, whose subnormal quotient by ANGULAR_TIE_DT is a tie for 19 of 31
    joints (tests/test_kinematics_hostile_host.py counts them)."""
    r = np.zeros((L, J, 4), np.float32)
    r[..., 3] = 1.0
    for j in range(J):
        row = np.zeros(4, np.float32)
        row[j % 3], row[(j + 1) % 3] = np.float32(7 * (2 * j + 1) * 2.0 ** -127), 1.0
        r[1::2, j] = row * np.float32(1 if j % 2 else -1)
    return r


def midpoint_rows(J, B):
    """(B, J, 4) rows (a, a', a'', W): W one of MIDPOINT_NORMS (the row's norm exactly, the imaginary parts being
    subnormal), the imaginary parts midpoint dividends of W, so every normalised imaginary part is a tie.  The root row
    is the identity."""
    q = np.zeros((B, J, 4), np.float32)
    for b in range(B):
        for j in range(J):
            W = MIDPOINT_NORMS[(b + j) % len(MIDPOINT_NORMS)]
            a = midpoint_dividends(W, 3 * (b + j) + 3)[-3:]
            q[b, j] = (a[0], -a[1], a[2], W if (b + j) % 3 else -W)
    q[:, 0] = (0.0, 0.0, 0.0, 1.0)
    return q


def gauss_nearest(v, w):
    """The oracle's smoothing filter (rtg_oracle.c gauss_nearest = scipy's gaussian_filter1d, mode 'nearest') over the
    frame axis -3 of raw velocities v (..., L, J, 3), taps w (2 R + 1) float64: the centre tap, then the tap pairs from
    the outermost inwards, in float64, rounded to float32 once.  tests/test_kinematics_hostile_host.py holds it to the
    oracle bit for bit."""
    v = np.asarray(v, np.float32)
    L, R = v.shape[-3], (len(w) - 1) // 2
    x = v.astype(np.float64)
    t = np.arange(L)

    def at(k):
        return np.take(x, np.clip(t + k, 0, L - 1), axis=-3)

    with np.errstate(all="ignore"):
        acc = x * w[R]
        for jj in range(-R, 0):
            acc = acc + (at(jj) + at(-jj)) * w[R + jj]
        return acc.astype(np.float32)


# ---- what the sequences reach, from oracle primitives (host)
def norm2_codes(q):
    """The float32 bits of |q|^2 minus 0x3F800000 for rows q (..., 4), the sum in the kernels' order: the near-unit
    table holds the codes -16 .. 16."""
    q = np.asarray(q, np.float32)
    with np.errstate(all="ignore"):
        n2 = ((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3]
    return np.ascontiguousarray(n2).view(np.int32).astype(np.int64) - 0x3F800000


def product_codes(r):
    """Per pair (t, t + 1) of r (L, J, 4): the code of |r[t+1] * conj(r[t])|^2 relative to 1.0f (its float32 bits minus
    0x3F800000), the index the kernels' near-unit table is looked up with; the product as oracle.quat_mul gives it and
    the sum in the kernels' order."""
    import oracle as orc
    a = np.ascontiguousarray(r[1:].reshape(-1, 4))
    b = np.ascontiguousarray((r[:-1] * np.float32([-1, -1, -1, 1])).reshape(-1, 4))
    with np.errstate(all="ignore"):
        return norm2_codes(orc.quat_mul(a, b))


def subnormal_quotients(raw_dt1, dt):
    """Of the raw velocities computed with dt = 1 (float32: the dividends themselves), (how many have a nonzero exact
    quotient by dt below 2^-126 -- the shared-reciprocal division's rare case --, how many of those round to a nonzero
    subnormal float32)."""
    a = np.asarray(raw_dt1, np.float32)
    with np.errstate(all="ignore"):
        exact = a.astype(np.float64) / np.float64(np.float32(dt))
        q = a / np.float32(dt)
    rare = np.isfinite(exact) & (exact != 0) & (np.abs(exact) < 2.0 ** -126)
    return int(rare.sum()), int((rare & (q != 0)).sum())

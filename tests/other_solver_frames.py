"""Hostile input frames for the UPPER_BODY, FULL_BODY_ROT and BODY_ROT solvers (a helper module: host numpy only, so
the CPU tests, the GPU tests and tools/make_golden.py build the same frames).

frames(kind) gives N0 = 4096 distinct deterministic frames laid out like tests/test_gpu_torso_fit.py: frames
[0, HEAD) mix the families within the waves, then each family has one whole 64-frame wave, and the rest are plain
rtg.synth poses.  FAMILIES[kind] is the table the host tests assert against the oracle: per family, whether every
frame of it raises ("all") or at least 48 of its 64 whole-wave frames do not ("few"), and whether its status-0
frames have finite DOFs.  rare_frames(kind) gives one ordinary frame and copies of it that differ in one rare-path
element each (tests/test_gpu_other_solvers.py::test_one_rare_element_per_group).

Quaternions are (x, y, z, w) rows; everything is built in float64 and rounded to float32 once.

Coupling to the oracle: the FULL_BODY_ROT families relative_identity, half_turn, gimbal and w_table_edges (and
fbp_wrist_frames) place a wrist relative to the wrist's parent rotation, which they take from the C oracle
(full_body_rot_wrist_parent), so those input rows follow the oracle's arm chain to the last bit.
tests/test_other_solvers_host.py requires the recorded fixture's inputs to equal freshly built ones; a later change to
the oracle's arm maps that moves a last bit fails that input comparison first, and the fixture is then to be recorded
again (tools/make_golden.py other_solvers_adversarial), not the comparison relaxed."""
import os

import numpy as np

from test_gpu_torso_fit import FAMILIES as TORSO_FAMILIES, _family_points

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UPPER_BODY, FULL_BODY_ROT, BODY_ROT = 1, 2, 3
NAMES = {UPPER_BODY: "upper_body", FULL_BODY_ROT: "full_body_rot", BODY_ROT: "body_rot"}
INPUTS = {UPPER_BODY: ("x",), FULL_BODY_ROT: ("body_rot", "body_pos", "lh", "rh"), BODY_ROT: ("global_rot",)}
N0, HEAD = 4096, 128
SEEDS = {UPPER_BODY: 9101, FULL_BODY_ROT: 9102, BODY_ROT: 9103}

# rows of the quaternion inputs the solvers read: FULL_BODY_ROT the shoulders' parents (17 left, 13 right) and the wrists
# (20, 16); BODY_ROT joints 18, 14 (YXZ) and 19, 15 (ZYX) with their parents 17, 13, 18, 14 (VTRDYN parent table)
READ_ROWS = {FULL_BODY_ROT: (13, 16, 17, 20), BODY_ROT: (13, 14, 15, 17, 18, 19)}
ARM_ROWS = tuple(range(13, 21))
SCALES_Q = (1e-12, 1e-20, 1e-40, 1e8, 1e18)
SCALES_P = (1e-30, 1e-12, 1e12, 1e25)
GIMBAL_OFF = (0.0, 1e-8, 1e-6, 1e-4)
F32 = np.float32
W_EDGES = [F32(v) for w in (1.0, -1.0, 0.0, 0.25) for v in
           (w, np.nextafter(F32(w), F32(-2)), np.nextafter(F32(w), F32(2))) if abs(float(v)) <= 1.0]

_QUAT_FAMILIES = [
    # name, raises, finite DOFs on its status-0 frames: (FULL_BODY_ROT, BODY_ROT)
    ("unit", ("few", "few"), (True, True)),
    ("nonunit", ("few", "few"), (True, True)),
    ("near_unit", ("few", "few"), (True, True)),
    ("negated", ("few", "few"), (True, True)),
    ("identity", ("few", "few"), (True, True)),
    ("relative_identity", ("few", "few"), (True, True)),
    ("half_turn", ("few", "few"), (True, True)),
    ("gimbal", ("few", "few"), (True, True)),
    ("w_table_edges", ("few", "few"), (True, True)),
    ("scale_1e-12", ("all", "few"), (True, True)),
    ("scale_1e-20", ("all", "few"), (True, True)),
    ("scale_1e-40", ("all", "all"), (True, True)),
    ("scale_1e8", ("few", "few"), (True, True)),
    ("scale_1e18", ("few", "all"), (True, True)),
    ("zero_row", ("all", "all"), (True, True)),
    ("nan", ("all", "all"), (True, True)),
    ("inf", ("all", "all"), (True, True)),
    ("signed_zero", ("few", "few"), (True, True)),
]
_ARM_FAMILIES = ["zero_length", "axis_arm", "straight_elbow", "folded_elbow"] + [f"pscale_{s:g}" for s in SCALES_P]


def _table(kind):
    t = []
    if kind == UPPER_BODY:
        for f in TORSO_FAMILIES:
            t.append(("torso_" + f, "all" if f in ("nan", "inf") else "few", True))
        t += [(f, "few", True) for f in _ARM_FAMILIES]
        t += [("nan_torso", "all", True), ("inf_torso", "all", True), ("negzero_torso", "few", True),
              ("nan_arm", "few", True), ("inf_arm", "few", True), ("negzero_arm", "few", True)]
    else:
        k = 0 if kind == FULL_BODY_ROT else 1
        t += [(n, r[k], fin[k]) for n, r, fin in _QUAT_FAMILIES]
        if kind == FULL_BODY_ROT:
            # a zero-length segment, a frame scaled to 1e-30 and a NaN / inf arm point end in a zero or NaN wrist-local
            # quaternion: scipy refuses it
            t += [(f, "all" if f in ("zero_length", "pscale_1e-30") else "few", True) for f in _ARM_FAMILIES]
            t += [("nan_arm", "all", True), ("inf_arm", "all", True), ("negzero_arm", "few", True),
                  ("gripper_threshold", "few", True)]
    return t


# per kind: [(family, "all" | "few", status-0 frames have finite DOFs)]
FAMILIES = {k: _table(k) for k in NAMES}


def plan(kind, i):
    """(family index or -1 for a plain frame, index of the frame within its family)."""
    nf = len(FAMILIES[kind])
    if i < HEAD:
        return i % nf, 64 + i // nf
    if i < HEAD + 64 * nf:
        return (i - HEAD) // 64, (i - HEAD) % 64
    return -1, 0


def wave(kind, family):
    """The frame indices of a family's whole wave."""
    k = [f[0] for f in FAMILIES[kind]].index(family)
    return np.arange(HEAD + 64 * k, HEAD + 64 * (k + 1))


# ---- float64 quaternion helpers (x, y, z, w)
def qmul(a, b):
    x1, y1, z1, w1 = a
    x2, y2, z2, w2 = b
    return np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2,
                     w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])


def qconj(a):
    return np.array([-a[0], -a[1], -a[2], a[3]])


def qrot(q, v):
    u, w = q[:3], q[3]
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def axis_quat(axis, angle):
    e = np.zeros(4)
    e[axis] = np.sin(angle / 2.0)
    e[3] = np.cos(angle / 2.0)
    return e


def euler_quat(seq, angles):
    """Intrinsic rotation about the axes named by seq ("YXZ": y, then the new x, then the new z)."""
    q = np.array([0.0, 0.0, 0.0, 1.0])
    for c, a in zip(seq, angles):
        q = qmul(q, axis_quat("XYZ".index(c), a))
    return q


def rand_unit(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return q * (1.0 if q[3] >= 0 else -1.0)


def gimbal_quat(seq, rng, j):
    """(a, +-pi/2 + off, c) in seq: exact gimbal lock and 1e-8, 1e-6, 1e-4 off it, both signs, cycling with j."""
    off = GIMBAL_OFF[j % 4] * (1.0 if (j // 8) % 2 == 0 else -1.0)
    mid = (np.pi / 2 if (j // 4) % 2 == 0 else -np.pi / 2) + off
    return euler_quat(seq, (rng.uniform(-np.pi, np.pi), mid, rng.uniform(-np.pi, np.pi)))


def w_edge_quat(rng, j):
    """A single-axis rotation whose w is 1, -1, 0, 0.25 or a float32 neighbour of one of them."""
    w = float(W_EDGES[j % len(W_EDGES)])
    q = np.zeros(4)
    q[(j // len(W_EDGES)) % 3] = np.sqrt(max(0.0, 1.0 - w * w))
    q[3] = w
    return q


def near_unit_factor(k):
    return np.sqrt(1.0 + k * 2.0 ** -23)


def _special(name, rng):
    return {"zero_row": 0.0, "nan": np.nan, "inf": rng.choice([np.inf, -np.inf]),
            "signed_zero": rng.choice([0.0, -0.0])}[name]


def _orc():
    import oracle as orc
    return orc


def _f32(a):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(a, np.float64).astype(np.float32)


def zero_pose():
    return np.load(os.path.join(GOLDEN, "zero_pose.npz"))


def full_body_rot_wrist_parent(q, p, l, r, side):
    """The oracle's wrist-parent rotation normalize(par * chain) of one FULL_BODY_ROT frame (side 0 left, 1 right),
    float32 bits: a wrist row set to it makes the Euler split's input conj(parent) * wrist have zero imaginary parts."""
    orc = _orc()
    ins = [np.ascontiguousarray(_f32(a)[None]) for a in (q, p, l, r)]
    _, lr = orc.full_body_rot(zero_pose()["vtrdyn_full_local_t"], *ins)
    c0 = 21 if side else 12
    chain = lr[:, c0]
    for j in (c0 + 1, c0 + 2, c0 + 3):
        chain = orc.quat_mul(chain, lr[:, j])
    return orc.quat_mul_norm(ins[0][:, 13 if side else 17], chain)[0].astype(np.float64)


def gripper_orig():
    """full_body_retargeter.py's open-hand x spread: mean over the five tips of zl[tip].x - zl[24].x, as the oracle sums it."""
    zl = zero_pose()["vtrdyn_full_local_t"]
    d = [F32(zl[g, 0]) - F32(zl[24, 0]) for g in (18, 22, 26, 30, 33)]
    return F32(F32(F32(F32(F32(d[0] + d[4]) + d[1]) + d[2]) + d[3]) / F32(5.0))


def _gripper_x(target):
    """The float32 x so that five tips at x (hand origin 0, identity wrist) give mean / orig == target exactly, or the
    closest reachable quotient."""
    orig = gripper_orig()
    x = F32(target) * orig
    best = None
    for _ in range(64):
        m = F32(F32(F32(F32(F32(x + x) + x) + x) + x) / F32(5.0))
        qv = F32(m / orig)
        if best is None or abs(float(qv) - float(target)) < best[0]:
            best = (abs(float(qv) - float(target)), x)
        if qv == F32(target):
            break
        # orig < 0: a larger x gives a smaller quotient
        up = (qv < F32(target)) != (orig < 0)
        x = np.nextafter(x, F32(np.inf) if up else F32(-np.inf))
    return best[1]


GRIPPER_TARGETS = [F32(0.7), np.nextafter(F32(0.7), F32(0)), np.nextafter(F32(0.7), F32(1)), F32(0.7) - F32(1e-3),
                   F32(0.7) + F32(1e-3)]


# ---- the families
def _arm_points(p, fam, j, rng, sh=(18, 14), el=(19, 15), wr=(20, 16)):
    """Point families of the arm rows of p (21, 3), in place."""
    if fam == "zero_length":
        s = (j // 2) % 2
        if j % 2 == 0:
            p[el[s]] = p[sh[s]]
        else:
            p[wr[s]] = p[el[s]]
    elif fam == "axis_arm":
        d = np.zeros(3)
        d[j % 3] = 0.3 if (j // 3) % 2 == 0 else -0.3
        for s in ((0, 1) if (j // 6) % 3 == 0 else ((j // 6) % 3 - 1,)):
            fore = p[wr[s]] - p[el[s]]
            p[el[s]] = p[sh[s]] + d
            p[wr[s]] = p[el[s]] + fore
    elif fam == "straight_elbow":
        for s in ((0, 1), (0,), (1,))[j % 3]:
            p[wr[s]] = p[el[s]] + (p[el[s]] - p[sh[s]])
    elif fam == "folded_elbow":
        for s in ((0, 1), (0,), (1,))[j % 3]:
            p[wr[s]] = p[sh[s]]
    else:
        raise KeyError(fam)


def _quat_family(kind, fam, q, j, rng, extra=None):
    """Quaternion families on q (21, 4) float64, in place.  Even j: the rows the solver reads (ARM_ROWS); odd j: all rows."""
    read = READ_ROWS[kind]
    rows = list(ARM_ROWS) if j % 2 == 0 else list(range(21))
    if fam == "unit":
        for r_ in rows:
            q[r_] = rand_unit(rng)
    elif fam == "nonunit":
        for r_ in rows:
            q[r_] *= rng.uniform(0.5, 2.0)
    elif fam == "near_unit":
        for r_ in rows:
            q[r_] *= near_unit_factor(int(rng.integers(-40, 41)))
    elif fam == "negated":
        for r_ in (rows if j % 4 < 2 else [read[(j // 4) % len(read)]]):
            q[r_] = -q[r_]
    elif fam == "identity":
        for r_ in rows:
            q[r_] = (0.0, 0.0, 0.0, 1.0)
    elif fam.startswith("scale_"):
        q[rows] *= float(fam[6:])
    elif fam in ("zero_row", "nan", "inf", "signed_zero"):
        r_ = read[int(rng.integers(len(read)))]
        if fam == "zero_row":
            q[r_] = 0.0
        else:
            q[r_, int(rng.integers(4))] = _special(fam, rng)
    elif kind == BODY_ROT:
        # relative rotations: child = parent * rel for the shoulders 18 / 14 (YXZ) and the elbows 19 / 15 (ZYX)
        joints = ((18, 17, "YXZ"), (14, 13, "YXZ"), (19, 18, "ZYX"), (15, 14, "ZYX"))
        pick = joints if j % 5 == 0 else (joints[j % 4],)
        for c, p_, seq in sorted(pick, key=lambda t: t[0] in (19, 15)):   # the shoulders first: the elbows hang on them
            if fam == "relative_identity":
                rel = np.array([0.0, 0.0, 0.0, 1.0])
            elif fam == "half_turn":
                rel = axis_quat(j % 3, np.pi) if j % 4 != 3 else np.append(_unit3(rng), 0.0)
            elif fam == "gimbal":
                rel = gimbal_quat(seq, rng, j)
            elif fam == "w_table_edges":
                rel = w_edge_quat(rng, j)
                if j % 2:
                    q[p_] = (0.0, 0.0, 0.0, 1.0)     # the link's w is then the edge value itself
            else:
                raise KeyError(fam)
            q[c] = qmul(q[p_], rel)
    else:
        # FULL_BODY_ROT: wrist = (par * chain) * rel, the wrist's parent rotation taken from the oracle
        for s in ((0, 1), (0,), (1,))[j % 3]:
            par = extra(s)
            if fam == "relative_identity":
                rel = np.array([0.0, 0.0, 0.0, 1.0])
            elif fam == "half_turn":
                rel = axis_quat(j % 3, np.pi) if j % 4 != 3 else np.append(_unit3(rng), 0.0)
            elif fam == "gimbal":
                rel = gimbal_quat("XYZ", rng, j)
            elif fam == "w_table_edges":
                rel = w_edge_quat(rng, j)
            else:
                raise KeyError(fam)
            q[16 if s else 20] = qmul(par, rel)


def _unit3(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _point_special(fam, rng):
    return {"nan": np.nan, "inf": rng.choice([np.inf, -np.inf]), "negzero": -0.0}[fam.split("_")[0]]


def _upper_frame(x, fam, j, rng, Zt):
    sgn = np.array([-1.0, -1.0, 1.0])   # coord_transform's flip: the solver sees x * sgn
    if fam.startswith("torso_"):
        x[10] = 0.0
        x[[17, 13, 11]] = _family_points(fam[6:], Zt, rng).astype(np.float64) * sgn
    elif fam in ("zero_length", "axis_arm", "straight_elbow", "folded_elbow"):
        _arm_points(x, fam, j, rng)
    elif fam.startswith("pscale_"):
        x *= float(fam[7:])
    elif fam.endswith("_torso"):
        x[(17, 13, 11, 10)[j % 4], int(rng.integers(3))] = _point_special(fam, rng)
    elif fam.endswith("_arm"):
        x[(18, 19, 20, 14, 15, 16)[j % 6], int(rng.integers(3))] = _point_special(fam, rng)
    else:
        raise KeyError(fam)


def _fbr_frame(q, p, l, r, fam, j, rng):
    if fam in ("zero_length", "axis_arm", "straight_elbow", "folded_elbow"):
        _arm_points(p, fam, j, rng)
    elif fam.startswith("pscale_"):
        s = float(fam[7:])
        p *= s
        l *= s
        r *= s
    elif fam.endswith("_arm"):
        p[(18, 19, 20, 14, 15, 16)[j % 6], int(rng.integers(3))] = _point_special(fam, rng)
    elif fam == "gripper_threshold":
        t = GRIPPER_TARGETS[j % 5]
        for s, (h, wrow) in enumerate(((l, 20), (r, 16))):
            if (j // 5) % 3 == 1 + s:
                continue                              # this side keeps its ordinary hand
            tips = [3, 7, 11, 15, 19]
            if (j // 15) % 2 == 0:
                # identity wrist, hand origin 0, every tip at the same x: the quotient is exactly the target
                q[wrow] = (0.0, 0.0, 0.0, 1.0)
                h[0] = 0.0
                h[tips, 0] = float(_gripper_x(t))
            else:
                # any wrist rotation: tip offsets (x, jitter) turned by its conjugate; the quotient lands near the target
                off = np.zeros((5, 3))
                off[:, 0] = float(t) * float(gripper_orig())
                off[:, 1:] = rng.normal(0.0, 0.02, (5, 2))
                w = q[wrow] / np.linalg.norm(q[wrow])
                h[tips] = h[0] + np.stack([qrot(qconj(w), o) for o in off])
    else:
        _quat_family(FULL_BODY_ROT, fam, q, j, rng, extra=lambda s: full_body_rot_wrist_parent(q, p, l, r, s))


_CACHE = {}


def frames(kind):
    """dict of the kind's N0 input arrays (float32) plus "family": the family index of every frame (-1: plain)."""
    if kind in _CACHE:
        return _CACHE[kind]
    from rtg import synth
    rng = np.random.default_rng(SEEDS[kind])
    fam_of = np.array([plan(kind, i)[0] for i in range(N0)], np.int16)
    names = [f[0] for f in FAMILIES[kind]]
    if kind == UPPER_BODY:
        ins = [synth.synth_upper_body_inputs(N0, SEEDS[kind]).astype(np.float64)]
        Zt = zero_pose()["vtrdyn_local_t"][[17, 13, 11]]
    elif kind == FULL_BODY_ROT:
        ins = [a.astype(np.float64) for a in synth.synth_full_body_rot_inputs(N0, SEEDS[kind])]
    else:
        ins = [synth.synth_body21_pose(N0, SEEDS[kind])[1].astype(np.float64)]
    for i in range(N0):
        k, j = plan(kind, i)
        if k < 0:
            continue
        if kind == UPPER_BODY:
            _upper_frame(ins[0][i], names[k], j, rng, Zt)
        elif kind == FULL_BODY_ROT:
            _fbr_frame(ins[0][i], ins[1][i], ins[2][i], ins[3][i], names[k], j, rng)
        else:
            _quat_family(BODY_ROT, names[k], ins[0][i], j, rng)
    out = {key: np.ascontiguousarray(_f32(a)) for key, a in zip(INPUTS[kind], ins)}
    out["family"] = fam_of
    _CACHE[kind] = out
    return out


def oracle_run(kind, d):
    """(dof, local_rot) of the C oracle for the kind's inputs d."""
    orc = _orc()
    zp = zero_pose()
    if kind == UPPER_BODY:
        return orc.upper_body(zp["vtrdyn_local_t"], d["x"])
    if kind == FULL_BODY_ROT:
        return orc.full_body_rot(zp["vtrdyn_full_local_t"], d["body_rot"], d["body_pos"], d["lh"], d["rh"])
    from rtg import assets
    return orc.body_rot(assets.parents("vtrdyn"), d["global_rot"])


def rare_frames(kind):
    """(ordinary frame, [(name, frame)]): frames are tuples of the kind's float32 input rows; each named frame equals
    the ordinary one except for one rare-path element (one joint, one link, one norm; the left or the right side)."""
    from rtg import synth
    rng = np.random.default_rng(SEEDS[kind] + 1)
    if kind == UPPER_BODY:
        base = [synth.synth_upper_body_inputs(4, 515)[2].astype(np.float64)]
    elif kind == FULL_BODY_ROT:
        base = [a[2].astype(np.float64) for a in synth.synth_full_body_rot_inputs(4, 515)]
    else:
        base = [synth.synth_body21_pose(4, 515)[1][2].astype(np.float64)]
    out = []

    def add(name, edit):
        f = [a.copy() for a in base]
        edit(*f)
        out.append((name, tuple(_f32(a) for a in f)))

    if kind == UPPER_BODY:
        Zt = zero_pose()["vtrdyn_local_t"][[17, 13, 11]]
        for j, side in ((0, "left"), (2, "right")):
            add(f"zero-length upper arm, {side}", lambda x, j=j: _arm_points(x, "zero_length", j, rng))
            add(f"zero-length forearm, {side}", lambda x, j=j: _arm_points(x, "zero_length", j + 1, rng))
        for ax in range(6):
            for s, side in ((1, "left"), (2, "right")):
                add(f"upper arm along axis {ax}, {side}", lambda x, j=ax + 6 * s: _arm_points(x, "axis_arm", j, rng))
        for j, side in ((1, "left"), (2, "right")):
            add(f"straight elbow, {side}", lambda x, j=j: _arm_points(x, "straight_elbow", j, rng))
            add(f"folded elbow, {side}", lambda x, j=j: _arm_points(x, "folded_elbow", j, rng))
        for fam in ("zero", "collinear", "mirrored", "tiny", "zero_plane"):
            add(f"torso {fam}", lambda x, fam=fam: _upper_frame(x, "torso_" + fam, 0, rng, Zt))
        return tuple(_f32(a) for a in base), out
    if kind == BODY_ROT:
        joints = ((18, 17, "YXZ", "left shoulder"), (14, 13, "YXZ", "right shoulder"), (19, 18, "ZYX", "left elbow"),
                  (15, 14, "ZYX", "right elbow"))
        for c, p_, seq, nm in joints:
            for j in range(16):
                def ed(g, c=c, p_=p_, seq=seq, j=j):
                    g[c] = qmul(g[p_], gimbal_quat(seq, rng, j))
                add(f"gimbal {nm} #{j}", ed)
            for j in range(len(W_EDGES) * 3):
                def ed(g, c=c, p_=p_, j=j):
                    g[c] = qmul(g[p_], w_edge_quat(rng, j))
                add(f"w edge {nm} #{j}", ed)
            for k in range(-40, 41, 3):
                def ed(g, c=c, k=k):
                    g[c] *= near_unit_factor(k)
                add(f"norm {nm} k={k}", ed)
        return tuple(_f32(a) for a in base), out
    par = [full_body_rot_wrist_parent(*base, s) for s in (0, 1)]
    for s, nm in ((0, "left"), (1, "right")):
        wrow, prow = (16, 13) if s else (20, 17)
        for j in range(16):
            def ed(q, p, l, r, j=j, s=s, wrow=wrow):
                q[wrow] = qmul(par[s], gimbal_quat("XYZ", rng, j))
            add(f"gimbal {nm} wrist #{j}", ed)
        for j in range(len(W_EDGES) * 3):
            def ed(q, p, l, r, j=j, s=s, wrow=wrow):
                q[wrow] = qmul(par[s], w_edge_quat(rng, j))
            add(f"w edge {nm} wrist #{j}", ed)

        def ed(q, p, l, r, s=s, wrow=wrow):
            q[wrow] = par[s]
        add(f"relative identity {nm} wrist", ed)
        # every code of |q|^2 around the near-unit table and both of its edges, on the parent row and on the wrist row
        for k in range(-40, 41):
            for row, rn in ((prow, "parent"), (wrow, "wrist")):
                def ed(q, p, l, r, k=k, row=row):
                    q[row] *= near_unit_factor(k)
                add(f"norm {nm} {rn} k={k}", ed)
        for t in GRIPPER_TARGETS:
            def ed(q, p, l, r, t=t, s=s, wrow=wrow):
                h = r if s else l
                q[wrow] = (0.0, 0.0, 0.0, 1.0)
                h[0] = 0.0
                h[[3, 7, 11, 15, 19], 0] = float(_gripper_x(t))
            add(f"gripper quotient {float(t)!r} {nm}", ed)
    return tuple(_f32(a) for a in base), out


# ---- FULL_BODY_POS: wrists whose local rotation sends the XYZ Euler split down its declined path
FBP_WRIST_N = 512


def fbp_wrist_frames():
    """(body, lh, rh) float32: FBP_WRIST_N synthetic FULL_BODY_POS frames whose five wrist-fit points are the zero-pose
    hand vectors turned by (wrist parent) * rel, the parent taken from the oracle (it does not depend on the hands).
    rel is a rotation about one axis -- identity, half turns, the w edges, random angles -- so the wrist's local
    quaternion conj(parent) * fit is a single-axis rotation up to the fit's ~1e-8 of rounding: the fast split meets
    components at that size, where its rounding margin fails, and the restatement's first and third angle cancel."""
    if "fbp" in _CACHE:
        return _CACHE["fbp"]
    from rtg import synth
    orc = _orc()
    zp = zero_pose()
    zl, zg = zp["vtrdyn_full_local_t"], zp["vtrdyn_full_global_t"]
    body, lh, rh = (a.astype(np.float64) for a in synth.synth_full_body_inputs(FBP_WRIST_N, 9104))
    _, lr, br = orc.full_body_pos(zl, zg, _f32(body), _f32(lh), _f32(rh), True)
    rng = np.random.default_rng(9105)
    fit = [2, 6, 10, 14, 17]
    for side, (h, z_rows, c0) in enumerate(((lh, [16, 20, 24, 28, 32], 12), (rh, [41, 45, 49, 53, 56], 21))):
        chain = lr[:, c0]
        for j in (c0 + 1, c0 + 2, c0 + 3):
            chain = orc.quat_mul(chain, lr[:, j])
        par = orc.quat_mul_norm(br[:, 10], chain).astype(np.float64)
        Z = zl[z_rows].astype(np.float64)
        for i in range(FBP_WRIST_N):
            j = i + 3 * side
            kind = j % 4
            if kind == 0:
                rel = np.array([0.0, 0.0, 0.0, 1.0])
            elif kind == 1:
                rel = axis_quat((j // 4) % 3, np.pi if (j // 12) % 2 == 0 else -np.pi)
            elif kind == 2:
                rel = w_edge_quat(rng, j // 4)
            else:
                rel = axis_quat((j // 4) % 3, rng.uniform(-np.pi, np.pi))
            t = qmul(par[i], rel)
            t /= np.linalg.norm(t)
            h[i, fit] = h[i, 0] + np.stack([qrot(t, z) for z in Z])
    out = tuple(np.ascontiguousarray(_f32(a)) for a in (body, lh, rh))
    _CACHE["fbp"] = out
    return out

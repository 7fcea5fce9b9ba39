"""Input frames and the oracle composition for the zero-pose transform (a helper module, not a test module: host numpy
only, so tools/make_golden_zero_pose.py, tests/test_rot_ingest_host.py and tests/test_gpu_rot_ingest.py build the same
frames).

The transform is out[f, j] = quat_mul_norm(quat_mul_norm(q[f, src[j]], pre), post[j]) (retarget/utils/parse_mocap.py:
65-134).  compose() states it with the C oracle's quat_mul_norm, twice; the host tests tie that to the reference's
recorded outputs bit for bit, the GPU tests hold the kernel to it.

family_frames(J) gives PER_FAMILY frames of each of the 18 quaternion families of tests/other_solver_frames.py
(_quat_family, BODY_ROT's joints: nothing there depends on the solver's output).  For J = 59 the family is applied to the
21 body joints' rows (BODY21_IN_FULL59) and the other 38 rows are random unit quaternions."""
import numpy as np

import oracle as orc
import other_solver_frames as osf
from retarget_to_ref import bits, conj, qmn  # noqa: F401  (re-exported for the two test files)

FAMILY_NAMES = [f[0] for f in osf._QUAT_FAMILIES]
PER_FAMILY = 8
BODY23_TO_21 = [0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22]
BODY21_IN_FULL59 = [0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 34, 35, 36, 37, 38, 39, 11, 12, 13, 14]
HALF_PI = np.pi / 2
# the four arm joints turned a quarter turn (parse_mocap.py:73-76, :98-101): joint, angle, axis
T2ZERO_EDITS = {
    "vtrdyn": ((18, -HALF_PI, 0), (19, -HALF_PI, 2), (14, HALF_PI, 0), (15, HALF_PI, 2)),
    "vtrdyn_full": ((12, -HALF_PI, 0), (13, -HALF_PI, 2), (37, HALF_PI, 0), (38, HALF_PI, 2)),
}
SEEDS = {"unit": 7301, "family": 7302, "broadcast": 7303}


def unit_rows(rng, shape):
    q = rng.normal(size=tuple(shape) + (4,))
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def unit_frames(n, J, seed=SEEDS["unit"]):
    return osf._f32(unit_rows(np.random.default_rng(seed + J), (n, J)))


def family_frame(fam, j, rng, J=21):
    """One frame (J, 4) float32 of family `fam`, variant j (even: the arm rows, odd: all rows; other_solver_frames)."""
    q = unit_rows(rng, (J,))
    if J == 21:
        osf._quat_family(osf.BODY_ROT, fam, q, j, rng)
    else:
        body = q[BODY21_IN_FULL59].copy()
        osf._quat_family(osf.BODY_ROT, fam, body, j, rng)
        q[BODY21_IN_FULL59] = body
    return osf._f32(q)


def family_frames(J, per=PER_FAMILY, seed=SEEDS["family"]):
    """(18 per, J, 4) float32: `per` frames of every family, family k at rows [k per, (k + 1) per)."""
    rng = np.random.default_rng(seed + J)
    return np.stack([family_frame(fam, j, rng, J) for fam in FAMILY_NAMES for j in range(per)])


def broadcast_frames(n=64, seed=SEEDS["broadcast"]):
    """(n, 23, 4) float32 raw broadcast rows: unit quaternions; frames 0-7 carry a zero row, a NaN, an inf, a negated
    row, w = -1, a -0 component, and a NaN in each of the two rows the 23 -> 21 gather drops (4 and 8)."""
    q = unit_frames(n, 23, seed)
    q[0, 11] = 0.0
    q[1, 12, 1] = np.nan
    q[2, 13, 2] = np.inf
    q[3, 14] = -q[3, 14]
    q[4, 15] = (0.0, 0.0, 0.0, -1.0)
    q[5, 16, 0] = -0.0
    q[6, 4, 3] = np.nan
    q[7, 8, 0] = np.nan
    return q


def compose(q, src, pre, post):
    """The oracle composition: q (B, J_in, 4), src (J_out) or None, pre (4), post (J_out, 4) -> (B, J_out, 4)."""
    q = np.ascontiguousarray(q, np.float32)
    rows = q if src is None else q[:, np.asarray(src)]
    if not rows.shape[0]:
        return np.zeros(rows.shape, np.float32)
    return qmn(qmn(rows, np.asarray(pre, np.float32)), np.asarray(post, np.float32))


def axis_quat(angle, axis):
    """The oracle's quat_from_angle_axis of f32(angle) about a coordinate axis, (4,) float32."""
    e = np.zeros((1, 3), np.float32)
    e[0, axis] = 1.0
    return orc.quat_from_angle_axis(np.array([angle], np.float32), e)[0]


def t2zero_from_assets(asset):
    """The t2zero rows rebuilt from oracle FK over the committed asset: identity local rotations with four joints set
    (rebuild_pose_by_local_rotation -> cal_forward_kinematics, kinematics.py:13-39)."""
    from retarget_to_ref import asset as load
    a = load(asset)
    J = len(a["parent_indices"])
    lr = np.tile(np.array([0, 0, 0, 1], np.float32), (1, J, 1))
    for j, angle, axis in T2ZERO_EDITS[asset]:
        lr[0, j] = axis_quat(angle, axis)
    g_rot, _ = orc.fk(np.asarray(a["parent_indices"], np.int32), np.asarray(a["local_translation"], np.float32), lr,
                      np.zeros((1, 3), np.float32))
    return g_rot[0]


def pad(frames, B, start=0):
    """B frames cycled from `frames`, beginning at `start`."""
    idx = (np.arange(B) + start) % len(frames)
    return np.ascontiguousarray(frames[idx])

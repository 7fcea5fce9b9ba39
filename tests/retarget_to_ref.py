"""Test-side reference of ``SkeletonState.retarget_to`` (poselib skeleton3d.py:742-889): the plan tables in plain
Python and the per-frame stages composed from oracle primitives (``oracle.state_fk``, ``state_local_rotation``,
``quat_mul_norm``, ``quat_normalize``, ``quat_rotate``).  tests/test_retarget_to_host.py ties it to the reference's
recorded outputs bit for bit; tests/test_gpu_retarget_to.py then holds the GPU to it.  Not a test module."""
import json
import os

import numpy as np

import oracle as orc
from conftest import GOLDEN, golden


def reduce_tree(parents, keep):
    """drop_nodes_by_names (:226-259): the kept joints in tree order, each hung from its nearest kept ancestor.
    Returns (kept indices, reduced parents)."""
    keep = set(int(k) for k in keep)
    kept = [j for j in range(len(parents)) if j in keep]
    new_index = {j: i for i, j in enumerate(kept)}
    red = []
    for j in kept:
        p = int(parents[j])
        while p != -1 and p not in keep:
            p = int(parents[p])
        assert p != -1 or int(parents[j]) == -1, "the root node cannot be dropped"
        red.append(-1 if p == -1 else new_index[p])
    return kept, red


def plan_tables(src_parents, tgt_parents, src_joint, tgt_joint):
    """kept_s, S_red parents, kept_t, T_red parents, perm, src_of of a mapping given as index pairs."""
    kept_s, sred = reduce_tree(src_parents, src_joint)
    kept_t, tred = reduce_tree(tgt_parents, tgt_joint)
    src_for = {int(t): int(s) for s, t in zip(src_joint, tgt_joint)}
    perm = [kept_s.index(src_for[t]) for t in kept_t]                  # _remapped_to, :721-740
    src_of = []
    for j in range(len(tgt_parents)):                                  # :876-880
        while j not in src_for:
            j = int(tgt_parents[j])
        src_of.append(kept_t.index(j))
    return kept_s, sred, kept_t, tred, perm, src_of


def _flat(fn, *xs):
    shape = xs[0].shape[:-1]
    args = [np.ascontiguousarray(np.broadcast_to(x, shape + x.shape[-1:]), np.float32).reshape(-1, x.shape[-1])
            for x in xs]
    if not args[0].shape[0]:
        return np.zeros(shape + (3 if fn is orc.quat_rotate else 4,), np.float32)
    return fn(*args).reshape(shape + (-1,))


def qnorm(q):
    return _flat(orc.quat_normalize, q)


def qmn(a, b):
    shape = np.broadcast_shapes(a.shape, b.shape)
    return _flat(orc.quat_mul_norm, np.broadcast_to(a, shape), np.broadcast_to(b, shape))


def conj(q):
    return (q * np.array([-1, -1, -1, 1], np.float32)).astype(np.float32)


def ident(n):
    return np.tile(np.array([0, 0, 0, 1], np.float32), (n, 1))


class Plan:
    """The constants of one retarget_to call.  src / tgt: (parents, tree_quat (J,4)); the t-poses as handed to
    retarget_to (normalised here, as from_rotation_and_root_translation does)."""

    def __init__(self, src, tgt, src_joint, tgt_joint, src_tpose_rot, src_tpose_root_t, tgt_tpose_rot,
                 tgt_tpose_root_t, R, scale):
        self.sp, self.stq = np.asarray(src[0], np.int32), np.asarray(src[1], np.float32)
        self.tp, self.ttq = np.asarray(tgt[0], np.int32), np.asarray(tgt[1], np.float32)
        (self.kept_s, self.sred, self.kept_t, self.tred, self.perm, self.src_of) = plan_tables(
            self.sp, self.tp, src_joint, tgt_joint)
        self.K = len(self.kept_s)
        self.R = np.asarray(R, np.float32).reshape(4)
        self.scale = np.float32(scale)
        self.tgt_root = np.asarray(tgt_tpose_root_t, np.float32).reshape(3)
        G_tp, self.t_tp = self.to_reduced_target(qnorm(np.asarray(src_tpose_rot, np.float32))[None],
                                                 np.asarray(src_tpose_root_t, np.float32).reshape(1, 3), True)
        self.cG_tp = conj(G_tp[0])
        Jt = len(self.tp)
        tg, _ = orc.state_fk(self.tp, self.ttq, np.zeros((Jt, 3), np.float32),
                             qnorm(np.asarray(tgt_tpose_rot, np.float32))[None], np.zeros((1, 3), np.float32))
        self.TG = tg[0][self.kept_t]

    def to_reduced_target(self, rot, root_t, is_local):
        """Stages 1-6: the state's global rotations on T_red (B,K,4) and the rotated root translation (B,3)."""
        rot, root_t = np.ascontiguousarray(rot, np.float32), np.ascontiguousarray(root_t, np.float32)
        B, Js, K = rot.shape[0], len(self.sp), self.K
        Gs = orc.state_fk(self.sp, self.stq, np.zeros((Js, 3), np.float32), rot, root_t)[0] if is_local else rot
        g = qnorm(Gs[:, self.kept_s])
        l = orc.state_local_rotation(np.asarray(self.sred, np.int32), ident(K), g)
        l = qnorm(l[:, self.perm])
        l[:, 0] = qmn(self.R, l[:, 0])
        l = qnorm(l)
        t = _flat(orc.quat_rotate, np.broadcast_to(self.R, (B, 4)), root_t)
        G = orc.state_fk(np.asarray(self.tred, np.int32), ident(K), np.zeros((K, 3), np.float32), l, t)[0]
        return G, t

    def __call__(self, rot, root_t, is_local):
        """-> the target state's local rotations (B,J_t,4) and root translation (B,3)."""
        B = len(rot)
        if B == 0:
            return np.zeros((0, len(self.tp), 4), np.float32), np.zeros((0, 3), np.float32)
        G, t = self.to_reduced_target(rot, root_t, is_local)
        n = qmn(qmn(G, self.cG_tp), self.TG)
        o = qnorm(n[:, self.src_of])
        out = qnorm(orc.state_local_rotation(self.tp, self.ttq, o))
        root = (self.tgt_root + (t - self.t_tp[0]) * self.scale).astype(np.float32)
        return out, root


def bits(a):
    """NaN-aware bit view: every NaN reads alike (its sign / payload differs between x86 and the GPU)."""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


FIXTURE_CASES = ("vtrdyn_hu_v5_local", "vtrdyn_hu_v5_global", "vtrdyn_full_hu", "noitom_hu_v5", "hu_v5_identity")
_CACHE = {}


def fixture():
    if "d" not in _CACHE:
        _CACHE["d"] = golden("retarget_to")
        with open(os.path.join(GOLDEN, "retarget_to_names.json")) as f:
            _CACHE["names"] = json.load(f)
    return _CACHE["d"], _CACHE["names"]


def asset(name):
    pkg = os.path.join(os.path.dirname(GOLDEN), os.pardir, "humanoid-real-time-retarget_amd", "assets")
    return np.load(os.path.join(pkg, f"{name}.npz"))


def fixture_plan(tag):
    """(Plan, names entry) of one fixture case, computed once."""
    if tag not in _CACHE:
        d, names = fixture()
        e = names[tag]
        s, t = asset(e["source"]), asset(e["target"])
        sj = [e["source_names"].index(a) for a in e["mapping"]]
        tj = [e["target_names"].index(b) for b in e["mapping"].values()]
        _CACHE[tag] = (Plan((s["parent_indices"], s["quat"]), (t["parent_indices"], t["quat"]), sj, tj,
                            d[f"{tag}_src_tpose_rot"], d[f"{tag}_src_tpose_root_t"], d[f"{tag}_tgt_tpose_rot"],
                            d[f"{tag}_tgt_tpose_root_t"], d[f"{tag}_R"], float(d[f"{tag}_scale"].reshape(-1)[0])), e)
    return _CACHE[tag]

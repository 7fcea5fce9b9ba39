"""Test-side restatement of the keypoint-target launch (rtg.h rtg_fit_targets_*): the host tables in plain Python and the
per-frame rule in float32 numpy, every operation one float32 rounding.  torch.linalg.norm's
sqrt(fma(z, z, fma(y, y, x x))) needs a fused multiply-add numpy does not have: ``fma32`` computes it in float64 with
the sum rounded to odd, which the final rounding to float32 then sees as the exact sum (53 >= 2 * 24 + 2 bits).
tests/test_fit_targets_host.py ties ``fma32`` to libm's fmaf and the rule to the reference's recorded
rescale_motion_to_standard_size; tests/test_gpu_fit_targets.py then holds the GPU to it.  Not a test module."""
import json
import os

import numpy as np

from conftest import GOLDEN

F32 = np.float32


def fma32(a, b, c):
    """fmaf(a, b, c) elementwise on float32 arrays: a b is exact in float64, the sum is rounded to odd there."""
    a, b, c = (np.asarray(x, F32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)   # TwoSum: s + e = p + c exactly
        fix = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def lnorm3(v):
    """torch.linalg.norm over the last axis of (..., 3) float32."""
    v = np.asarray(v, F32)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    with np.errstate(all="ignore"):
        return np.sqrt(fma32(z, z, fma32(y, y, x * x)))


def zero_pose_global(parents, local_t):
    """G: float32 sums taken parents first, G[root] = 0."""
    lt = np.asarray(local_t, F32).reshape(-1, 3)
    G = np.zeros_like(lt)
    for j in range(1, len(parents)):
        G[j] = G[int(parents[j])] + lt[j]
    return G


def tables(tgt_parents, tgt_local_t, src_joint, tgt_joint):
    """anchor (K; -1: the root pair), seg (K, 3), weight (J_t), src_of (J_t); pairs numbered as given."""
    Jt, K = len(tgt_parents), len(src_joint)
    pair_of = {int(t): k for k, t in enumerate(tgt_joint)}
    assert len(pair_of) == K and len(set(int(s) for s in src_joint)) == K and 0 in pair_of
    G = zero_pose_global(tgt_parents, tgt_local_t)
    src_of = []
    for j in range(Jt):
        while j not in pair_of:
            j = int(tgt_parents[j])
        src_of.append(pair_of[j])
    anchor, seg = np.full(K, -1, np.int32), np.zeros((K, 3), F32)
    for k, t in enumerate(tgt_joint):
        if int(t) == 0:
            continue
        anchor[k] = src_of[int(tgt_parents[int(t)])]
        seg[k] = G[int(t)] - G[int(tgt_joint[anchor[k]])]
    weight = np.array([1.0 if j in pair_of else 0.0 for j in range(Jt)], F32)
    return dict(anchor=anchor, seg=seg, weight=weight, src_of=np.array(src_of, np.int32))


def fit_targets(tgt_parents, tgt_local_t, src_joint, tgt_joint, src_pos, dir=None, root_scale=None, root_offset=None,
                tab=None):
    """src_pos (B, J_s, 3) -> (B, J_t, 3) float32 by the rule of rtg.h."""
    tab = tab or tables(tgt_parents, tgt_local_t, src_joint, tgt_joint)
    x = np.asarray(src_pos, F32)
    m = x if dir is None else x * np.asarray(dir, F32)
    out = np.zeros(x.shape[:1] + (len(tgt_parents), 3), F32)
    with np.errstate(all="ignore"):
        for k in np.argsort(np.asarray(tgt_joint)):   # ascending target index: anchors first
            s, t, a = int(src_joint[k]), int(tgt_joint[k]), int(tab["anchor"][k])
            if a < 0:
                r = m[:, s]
                if root_scale is not None:
                    r = r * np.asarray(root_scale, F32)
                if root_offset is not None:
                    r = r + np.asarray(root_offset, F32)
                out[:, t] = r
                continue
            d = m[:, s] - m[:, int(src_joint[a])]
            scale = lnorm3(d) / lnorm3(tab["seg"][k])
            out[:, t] = out[:, int(tgt_joint[a])] + d / scale[:, None]
        for j in range(len(tgt_parents)):
            out[:, j] = out[:, int(tgt_joint[tab["src_of"][j]])]
    return out


def limb_ratio(src_parents, src_local_t, tgt_parents, tgt_local_t, src_joint, tgt_joint, link):
    """Over the pairs on the path root -> link: the summed target |seg| over the same sum in the source zero pose."""
    tab = tables(tgt_parents, tgt_local_t, src_joint, tgt_joint)
    Gs = zero_pose_global(src_parents, src_local_t)
    k = int(tab["src_of"][int(link)])
    num = den = 0.0
    while tab["anchor"][k] >= 0:
        a = int(tab["anchor"][k])
        num += float(np.linalg.norm(tab["seg"][k].astype(np.float64)))
        den += float(np.linalg.norm((Gs[int(src_joint[k])] - Gs[int(src_joint[a])]).astype(np.float64)))
        k = a
    return num / den


def same_bits(a, b):
    """Bit for bit, every NaN alike (sign and payload of an arithmetic NaN differ between x86 and the GPU)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    nan = lambda v: np.where(np.isnan(v), np.uint32(0x7FC00000), v.view(np.uint32))
    return a.shape == b.shape and np.array_equal(nan(a), nan(b))


# ------------------------------------------------------------------ the cases both test modules share
def golden_mapping(case):
    """(source asset, target asset, src_joint, tgt_joint, names dict) of a mapping of tests/golden/retarget_to_names.json."""
    with open(os.path.join(GOLDEN, "retarget_to_names.json")) as f:
        c = json.load(f)[case]
    sj = [c["source_names"].index(s) for s in c["mapping"]]
    tj = [c["target_names"].index(t) for t in c["mapping"].values()]
    return c["source"], c["target"], np.array(sj, np.int32), np.array(tj, np.int32), c


def synthetic(kind, seed=0):
    """(src parents, src local_t, tgt parents, tgt local_t, src_joint, tgt_joint) of the synthetic trees."""
    rng = np.random.default_rng(seed)
    lt = lambda J: rng.normal(0, 0.3, (J, 3)).astype(F32)
    chain = lambda J: np.arange(-1, J - 1, dtype=np.int32)
    if kind == "chain64":        # fully mapped, the source joints permuted
        J = 64
        sj = np.concatenate([[0], 1 + rng.permutation(J - 1)]).astype(np.int32)
        return chain(J), lt(J), chain(J), lt(J), sj, np.arange(J, dtype=np.int32)
    if kind == "chain64_half":   # every second joint mapped
        J = 64
        tj = np.arange(0, J, 2, dtype=np.int32)
        return chain(J), lt(J), chain(J), lt(J), tj[::-1].copy(), tj
    if kind == "star60":
        J = 60
        par = np.concatenate([[-1], np.zeros(J - 1)]).astype(np.int32)
        tj = rng.permutation(J).astype(np.int32)
        return par, lt(J), par, lt(J), np.arange(J, dtype=np.int32), tj
    if kind == "j2":
        return chain(2), lt(2), chain(2), lt(2), np.array([1, 0], np.int32), np.array([0, 1], np.int32)
    if kind == "k1":             # only the root kept: 21 source joints, 33 target links
        par = np.concatenate([[-1], rng.integers(0, np.arange(1, 33))]).astype(np.int32)
        return chain(21), lt(21), par, lt(33), np.array([7], np.int32), np.array([0], np.int32)
    raise KeyError(kind)


# ------------------------------------------------------------------ the outcome recipe (CPU float64 loop and GPU)
HU_GROUPS = ((range(1, 13), 1.35), ((13,), 1.25), (range(14, 32), 1.2), ((32,), 1.25))   # legs, torso, arms, neck


def outcome_recipe(seed=1, B=64):
    """A "human" of other proportions posed like the robot: the 33-link Hu of tests/golden/fk_grad.npz (limits on),
    the human its own tree with the leg offsets x 1.35, the arm offsets x 1.2, torso and neck x 1.25.  Each angle is
    mid + 0.6 half U(-1, 1), the root yaw +-0.5 rad, the root position (N(0, 0.3), N(0, 0.3), 1.2).  The 15 links of
    the golden VTRDyn -> Hu mapping are observed.  -> a dict of float32 arrays and the skeleton."""
    import torch
    from test_fk_grad_host import dof_fk
    from test_pose_fit_host import _Hu
    s = _Hu()
    _, _, _, _, c = golden_mapping("vtrdyn_full_hu")
    links = np.array(sorted(c["target_names"].index(t) for t in c["mapping"].values()), np.int32)
    human_lt = np.array(s.lt, F32).copy()
    for joints, k in HU_GROUPS:
        human_lt[list(joints)] *= F32(k)
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(s.lo, np.float64), np.asarray(s.hi, np.float64)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    truth = (mid + 0.6 * half * rng.uniform(-1, 1, (B, s.J - 1))).astype(F32)
    yaw = rng.uniform(-0.5, 0.5, B)
    q_true = np.stack([0 * yaw, 0 * yaw, np.sin(yaw / 2), np.cos(yaw / 2)], -1).astype(F32)
    t_true = np.stack([rng.normal(0, 0.3, B), rng.normal(0, 0.3, B), np.full(B, 1.2)], -1).astype(F32)
    f64 = lambda a: torch.as_tensor(np.asarray(a)).to(torch.float64)
    par = [int(p) for p in s.par]
    with torch.no_grad():
        fk = lambda lt, t: dof_fk(f64(truth), f64(q_true), f64(t), par, f64(lt), s.axis, f64(s.lo), f64(s.hi))[1].numpy()
        human = fk(human_lt, t_true).astype(F32)
        robot0 = fk(s.lt, np.zeros_like(t_true))   # the truly posed robot, root at the origin
    w = np.zeros(s.J, F32)
    w[links] = 1
    ratio = limb_ratio(s.par, human_lt, s.par, s.lt, links, links, c["target_names"].index("left_ankle_link"))
    return dict(s=s, links=links, human_lt=human_lt, human=human, robot0=robot0, w=w, ratio=ratio, truth=truth,
                start=np.tile(mid.astype(F32), (B, 1)), q0=np.tile(np.array([0, 0, 0, 1], F32), (B, 1)),
                names=c["target_names"])


def outcome_error(x, dof, q, fitted=None):
    """Mean distance of the mapped links, root at the origin, from the truly posed robot."""
    import torch
    from test_fk_grad_host import dof_fk
    s = x["s"]
    f64 = lambda a: torch.as_tensor(np.asarray(a)).to(torch.float64)
    with torch.no_grad():
        q = f64(q)
        q = q / q.norm(dim=-1, keepdim=True)
        gp = dof_fk(f64(dof), q, torch.zeros(len(q), 3, dtype=torch.float64), [int(p) for p in s.par], f64(s.lt),
                    s.axis, f64(s.lo), f64(s.hi))[1].numpy()
    return float(np.linalg.norm(gp[:, x["links"]] - x["robot0"][:, x["links"]], axis=-1).mean())


_OUTCOME = {}


def outcome_float64():
    """The float64 loop (tests/test_pose_fit_host.py ref_pose_fit) on the recipe, raw keypoints against rescaled ones:
    128 Adam steps, every lr 0.02, both root blocks fitted, from mid-range angles, the identity and the root keypoint.
    -> dict(raw=(mean loss, error), rescaled=(mean loss, error)); computed once per session."""
    if not _OUTCOME:
        import torch
        from test_pose_fit_host import ref_pose_fit
        x = outcome_recipe()
        s = x["s"]
        r = F32(x["ratio"])
        targets = dict(raw=x["human"], rescaled=fit_targets(s.par, s.lt, x["links"], x["links"], x["human"],
                                                            root_scale=[r, r, r]))
        for k, tgt in targets.items():
            loss, a, q, _ = ref_pose_fit(s, x["start"], x["q0"], tgt[:, 0], tgt, x["w"], True, torch.float64, 3, 128,
                                         record=(128,))[128]
            _OUTCOME[k] = (float(loss.mean()), outcome_error(x, a, q))
    return _OUTCOME

"""The FK family (rtg_fk_f32, rtg_state_fk_f32, both inverse forms, the *_multi launches, rtg_dof_fk_f32's root rotation,
rtg_retarget_to_f32) on hostile rotations, bit for bit against the C oracle: the 18 quaternion families of
tests/kinematics_frames.py (unit, non-unit, near-unit rows whose squared norm is on, at the edge of and off the
near-unit table, negated, identity, half turns, gimbal, w edges, rows scaled by 1e-40 .. 1e18, zero / NaN / inf rows,
signed zeros), each on every row of a frame or on a random tenth of them, on Hu v5 (16 frames per wave), VTRDyn-59 (8),
a bushy 97-joint tree (the lane walk) and a one-joint chain.  tests/test_kinematics_hostile_host.py anchors the oracle
on these families to the reference's own outputs.

Every comparison is on the raw bits, every NaN reading alike (retarget_to_ref.bits)."""
import numpy as np
import pytest

import kinematics_frames as kf
from retarget_to_ref import bits
from test_gpu_parity import _dof_model, _random_tree, _topo

pytestmark = pytest.mark.gpu

PER_FAMILY = 32
TOPOS = ["hu_v5", "vtrdyn_full", "bushy97", "chain1"]
FRAMES_PER_WAVE = {"hu_v5": 16, "vtrdyn_full": 8, "bushy97": 64, "chain1": 16}   # forward FK; inverse FK: 8 (walk: 64)
_CACHE = {}


def topo(name):
    """(Topology, parents, local_t, tree_quat, rot (18 * 32, J, 4), root_t, family per frame), built once."""
    if name not in _CACHE:
        from rtg import assets
        from rtg.runtime import Topology
        if name in ("hu_v5", "vtrdyn_full"):
            par, lt, tq = assets.parents(name), assets.local_translation(name), assets.tree_quat(name)
            T = _topo(name)
        else:
            J = 97 if name == "bushy97" else 1
            rng = np.random.default_rng(J)
            par = _random_tree(rng, J, "bushy" if J > 1 else "chain")
            lt = rng.normal(0, 0.2, (J, 3)).astype(np.float32)
            tq = rng.normal(size=(J, 4))
            tq = (tq / np.linalg.norm(tq, axis=1, keepdims=True)).astype(np.float32)
            T = Topology(par, lt, tq)
        _CACHE[name] = (T, par, lt, tq) + kf.fk_rotations(len(par), PER_FAMILY)
    return _CACHE[name]


def _np(t):
    return t.detach().cpu().numpy()


def _check(got, want, fam, tag):
    bad = (bits(got) != bits(want)).reshape(len(want), -1).any(axis=1)
    if bad.any():
        who = [kf.FK_FAMILIES[k] for k in fam[bad]]
        count = {f: who.count(f) for f in dict.fromkeys(who)}
        raise AssertionError(f"{tag}: {int(bad.sum())} of {len(bad)} frames differ, by family {count}; first frames "
                             f"{np.flatnonzero(bad)[:6].tolist()}")


def _oracle_all(name, lr, rt):
    """The oracle's six outputs for frames lr, rt: FK and inverse FK, plain and SkeletonState form (the state forms on
    the rows as given: SkeletonState normalises them before, which the callers below do as well)."""
    import oracle as orc
    _, par, lt, tq = topo(name)[:4]
    with np.errstate(all="ignore"):
        gr, gp = orc.fk(par, lt, lr, rt)
        sr, sp = orc.state_fk(par, tq, lt, lr, rt)
        return dict(g_rot=gr, g_pos=gp, inv=orc.local_rotation(par, gr), s_rot=sr, s_pos=sp,
                    s_inv=orc.state_local_rotation(par, tq, sr))


def _gpu_all(name, lr, rt, g_rot, s_rot):
    from rtg import ops
    T = topo(name)[0]
    gr, gp = ops.forward_kinematics(T, lr, rt)
    sr, sp = ops.forward_kinematics(T, lr, rt, state=True)
    return dict(g_rot=_np(gr), g_pos=_np(gp), inv=_np(ops.local_rotation(T, g_rot)), s_rot=_np(sr), s_pos=_np(sp),
                s_inv=_np(ops.local_rotation(T, s_rot, state=True)))


@pytest.mark.parametrize("name", TOPOS)
def test_families_vs_oracle(gpu, name):
    """18 families x 32 frames in one batch through forward FK (plain and state=True, on the raw rows and on the rows
    normalised as SkeletonState stores them) and inverse FK (both forms, on the oracle's global rotations); then ragged
    batches that mix the families: 1, F - 1, F, F + 1 and 3 F + 5 frames for the forward tile's F and the inverse
    tile's 8."""
    import oracle as orc
    lr, rt, fam = topo(name)[4:]
    B, J = lr.shape[:2]
    with np.errstate(all="ignore"):
        nlr = orc.quat_normalize(lr.reshape(-1, 4)).reshape(B, J, 4)
    for tag, rows in (("raw", lr), ("normalised", nlr)):
        want = _oracle_all(name, rows, rt)
        got = _gpu_all(name, rows, rt, want["g_rot"], want["s_rot"])
        for k in want:
            _check(got[k], want[k], fam, f"{name} {tag} {k}")
    want = _oracle_all(name, lr, rt)
    F = FRAMES_PER_WAVE[name]
    for n in sorted({1, F - 1, F, F + 1, 3 * F + 5, 7, 8, 9, 29}):
        idx = (np.arange(n) * 37 + n) % B
        got = _gpu_all(name, lr[idx], rt[idx], want["g_rot"][idx], want["s_rot"][idx])
        for k in want:
            _check(got[k], want[k][idx], fam[idx], f"{name} B={n} {k}")


@pytest.mark.parametrize("name", TOPOS[:3])
def test_tie_normalisations(gpu, name):
    """Rows (a, a', a'', W) whose norm is W exactly and whose normalised imaginary parts are exact ties between two
    subnormal float32 values (kinematics_frames.midpoint_rows): the IEEE division rounds to even, a product by a rounded
    1 / W does not (the subnormal branch of the shared-reciprocal division in qnormalize)."""
    J = len(topo(name)[1])
    q = kf.midpoint_rows(J, 67)
    rt = np.zeros((len(q), 3), np.float32)
    want = _oracle_all(name, q, rt)
    got = _gpu_all(name, q, rt, want["g_rot"], want["s_rot"])
    for k in want:
        assert (bits(got[k]) == bits(want[k])).all(), f"{name} tie rows {k}: " \
            f"{int((bits(got[k]) != bits(want[k])).sum())} elements differ"
    sub = np.abs(want["g_rot"][:, 1:, :3])
    assert ((sub > 0) & (sub < np.float32(2.0 ** -126))).mean() > 0.5    # the global rotations carry subnormal parts


@pytest.mark.parametrize("names", [["hu_v5", "vtrdyn_full", "chain1"], TOPOS])
def test_kinematics_multi_mixes_families(gpu, names):
    """One rtg_kinematics_multi_f32 launch whose FK and inverse-FK segments each hold other families, at ragged sizes
    (lane groups for the three small trees; with the 97-joint tree every segment takes the lane walk); and the FK-only
    and inverse-only multi launches."""
    from rtg import ops
    sizes = [65, 576, 17, 130]
    fk, inv, want, fams = [], [], [], []
    for i, (name, n) in enumerate(zip(names, sizes)):
        lr, rt, fam = topo(name)[4:]
        idx = (np.arange(n) * 53 + 97 * i) % len(lr)
        w = _oracle_all(name, lr[idx], rt[idx])
        fk.append((topo(name)[0], lr[idx], rt[idx]))
        inv.append((topo(name)[0], w["g_rot"]))
        want.append(w)
        fams.append(fam[idx])
    fouts, iouts = ops.kinematics_multi(fk, inv)
    for name, (gr, gp), loc, w, fam in zip(names, fouts, iouts, want, fams):
        _check(_np(gr), w["g_rot"], fam, f"multi {name} g_rot")
        _check(_np(gp), w["g_pos"], fam, f"multi {name} g_pos")
        _check(_np(loc), w["inv"], fam, f"multi {name} inverse")
    for name, (gr, gp), w, fam in zip(names, ops.forward_kinematics_multi(fk), want, fams):
        _check(_np(gr), w["g_rot"], fam, f"fk_multi {name} g_rot")
        _check(_np(gp), w["g_pos"], fam, f"fk_multi {name} g_pos")
    for name, loc, w, fam in zip(names, ops.local_rotation_multi(inv), want, fams):
        _check(_np(loc), w["inv"], fam, f"local_rotation_multi {name}")


@pytest.mark.parametrize("tag,name", [("hu_clip", "hu"), ("hu_noclip", "hu"), ("hu_v5_noclip", "hu_v5")])
def test_dof_fk_root_rotation_families(gpu, tag, name):
    """HuForwardModel.forward_kinematics with the families on the root rotation (the row its kernel normalises through
    the near-unit table), random joint angles, clip on and off."""
    import oracle as orc
    from conftest import golden
    from rtg import assets, ops
    d = golden("dof_fk")
    model, lo, hi = _dof_model(d, tag, name)
    rr, rt, fam = kf.fk_rotations(1, PER_FAMILY, seed=3)
    rr = np.ascontiguousarray(rr[:, 0])
    dof = np.random.default_rng(31).uniform(-4, 4, (len(rr), model.num_dofs)).astype(np.float32)
    gr, gp = ops.dof_forward_kinematics(model, dof, rr, rt, clip=lo is not None)
    with np.errstate(all="ignore"):
        ogr, ogp = orc.dof_fk(assets.parents(name), assets.local_translation(name), d[f"{tag}_axis"], dof, rr, rt, lo, hi)
    _check(_np(gr), ogr, fam, f"{tag} g_rot")
    _check(_np(gp), ogp, fam, f"{tag} g_pos")


@pytest.mark.parametrize("case", ["vtrdyn_hu_v5_local", "vtrdyn_full_hu"])
def test_retarget_to_families(gpu, case):
    """retarget_to with the families on the source rows, local and global, against tests/retarget_to_ref.Plan: near_unit
    puts the kernel's first normalisation on the table, which test_gpu_retarget_to.random_frames keeps off it."""
    from rtg import ops
    from test_gpu_retarget_to import fixture_gpu_plan
    plan, gp = fixture_gpu_plan(case)
    q, t, fam = kf.fk_rotations(len(plan.sp), PER_FAMILY, seed=5)
    c = kf.norm2_codes(q[fam == kf.FK_FAMILIES.index("near_unit")][:PER_FAMILY // 2])
    assert (np.abs(c) < 16).any() and np.isin(np.abs(c), (16, 17)).any() and (np.abs(c) > 17).any()   # on, edge, off
    for local in (True, False):
        with np.errstate(all="ignore"):
            want_rot, want_root = plan(q, t, local)
        rot, root = ops.retarget_to(gp, q, t, local)
        _check(_np(rot), want_rot, fam, f"{case} local={local} rotations")
        _check(_np(root), want_root, fam, f"{case} local={local} root")


@pytest.mark.parametrize("name", TOPOS)
def test_fk_frames_are_isolated_and_runs_repeat(gpu, name):
    """A NaN frame and a frame with a zero row inside the middle tile of three (forward FK's tile, and the inverse's 8
    frames): every other frame keeps the clean run's bits, the bad frames equal the oracle, two runs give the same
    bits; forward and inverse FK, plain and state form."""
    lr, rt, fam = topo(name)[4:]
    unit = np.flatnonzero(fam == kf.FK_FAMILIES.index("unit"))[:PER_FAMILY // 2]
    for F in sorted({FRAMES_PER_WAVE[name], 8}):
        B = 3 * F
        idx = unit[np.arange(B) % len(unit)]
        q, t = lr[idx].copy(), rt[idx].copy()
        q += (np.arange(B, dtype=np.float32) * np.float32(1e-3))[:, None, None]   # distinct frames
        clean = _oracle_all(name, q, t)
        got0 = _gpu_all(name, q, t, clean["g_rot"], clean["s_rot"])
        a, b = F + 1, 2 * F - 2 if F > 3 else F + 2
        qd, td, gd, sd = q.copy(), t.copy(), clean["g_rot"].copy(), clean["s_rot"].copy()
        J = q.shape[1]
        qd[a], td[a], gd[a], sd[a] = np.nan, np.nan, np.nan, np.nan
        qd[b, J // 2], gd[b, J // 2], sd[b, J // 2] = 0.0, 0.0, 0.0
        want = _oracle_all(name, qd, td)
        import oracle as orc
        _, par, _, tq = topo(name)[:4]
        with np.errstate(all="ignore"):
            want["inv"], want["s_inv"] = orc.local_rotation(par, gd), orc.state_local_rotation(par, tq, sd)
        got1 = _gpu_all(name, qd, td, gd, sd)
        got2 = _gpu_all(name, qd, td, gd, sd)
        others = np.ones(B, bool)
        others[[a, b]] = False
        for k in want:
            assert (bits(got1[k]) == bits(got2[k])).all(), f"{name} F={F} {k}: two runs differ"
            assert (bits(got1[k])[others] == bits(got0[k])[others]).all(), f"{name} F={F} {k}: a clean frame moved"
            assert (bits(got1[k])[[a, b]] == bits(want[k])[[a, b]]).all(), f"{name} F={F} {k}: bad frames off the oracle"
            assert (bits(got0[k]) == bits(clean[k])).all(), f"{name} F={F} {k}: clean run off the oracle"
        assert np.isnan(got1["g_rot"][a]).all() and np.isnan(got1["inv"][a]).all()

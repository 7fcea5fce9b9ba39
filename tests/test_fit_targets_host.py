"""CPU-only checks of the keypoint targets for the pose fit (rtg_fit_targets_*): the symbols are there under ABI 7, every
rejection is decided before any device work with its own message (NULL handles, never-dereferenced addresses), the
Python entry points raise RtgError without a GPU, the library's host tables and ``ops.limb_ratio`` agree with the
restatement (tests/fit_targets_ref.py) on the shipped assets and on hand-made trees, the restatement with one tree and
the identity mapping IS the reference's recorded rescale_motion_to_standard_size, and the outcome the feature is for --
the float64 pose-fit loop lands far closer to the truly posed robot on rescaled keypoints than on raw ones."""
import ctypes
import re

import numpy as np
import pytest
import torch

import fit_targets_ref as ref
from conftest import REPO, golden

INVALID, UNSUPPORTED = 1, 4   # RTG_ERR_INVALID_ARGUMENT, RTG_ERR_UNSUPPORTED
GOLDEN_CASES = ("vtrdyn_full_hu", "vtrdyn_hu_v5_global", "noitom_hu_v5")
SYNTHETIC = ("chain64", "chain64_half", "star60", "j2", "k1")
IP, FP = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)


def _lib():
    from rtg import _lib
    return _lib.lib()


def _asset(name):
    from rtg import assets
    return assets.parents(name).astype(np.int32), assets.local_translation(name)


# ------------------------------------------------------------------ symbols
def test_symbols_and_abi_version():
    from rtg import _lib
    lib = _lib.lib()
    names = ("rtg_fit_targets_plan_create", "rtg_fit_targets_plan_destroy", "rtg_fit_targets_f32",
             "rtg_fit_targets_plan_tables")
    with open(f"{REPO}/include/rtg.h") as f:
        header = f.read()
    for n in names:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
        assert re.search(r"\bint\s+" + n + r"\s*\(", header), n   # the prototype
    assert re.search(r"#define\s+RTG_ABI_VERSION\s+7\b", header)
    assert lib.rtg_abi_version() == 7   # new symbols only: nothing that existed changed


# ------------------------------------------------------------------ rejections, before any device work
def _tables(Js, par, lt, sj, tj, K=None):
    par, sj, tj = (None if a is None else np.ascontiguousarray(a, np.int32) for a in (par, sj, tj))
    lt = None if lt is None else np.ascontiguousarray(lt, np.float32)
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)
    Jt = 0 if par is None else len(par)
    K = (0 if sj is None else len(sj)) if K is None else K
    return _lib().rtg_fit_targets_plan_tables(Js, p(par, IP), p(lt, FP), Jt, p(sj, IP), p(tj, IP), K, None, None, None,
                                              None)


CH4 = np.array([-1, 0, 1, 2], np.int32)
LT4 = np.ones((4, 3), np.float32)
CH65 = np.arange(-1, 64, dtype=np.int32)


@pytest.mark.parametrize("args, status, msg", [
    ((4, None, LT4, [0], [0]), INVALID, b"NULL parents/local_t"),
    ((4, CH4, None, [0], [0]), INVALID, b"NULL parents/local_t"),
    ((4, CH4, LT4, [], []), INVALID, b"the joint mapping is empty"),
    ((4, CH4, LT4, None, [0], 1), INVALID, b"the joint mapping is empty"),
    ((4, CH4, LT4, [0], None, 1), INVALID, b"the joint mapping is empty"),
    ((4, CH4, LT4, [0], [0], -1), INVALID, b"the joint mapping is empty"),
    ((4, CH4, LT4, [0, 4], [0, 1]), INVALID, b"pair 1 = (4, 1) is out of range"),
    ((4, CH4, LT4, [0, -1], [0, 1]), INVALID, b"pair 1 = (-1, 1) is out of range"),
    ((4, CH4, LT4, [0, 1], [0, 4]), INVALID, b"pair 1 = (1, 4) is out of range"),
    ((4, CH4, LT4, [0, 1], [0, -1]), INVALID, b"pair 1 = (1, -1) is out of range"),
    ((4, CH4, LT4, [0, 1, 1], [0, 1, 2]), INVALID, b"source joint 1 is named twice (pairs 1 and 2)"),
    ((4, CH4, LT4, [0, 1, 2], [0, 3, 3]), INVALID, b"target joint 3 is named twice (pairs 1 and 2)"),
    ((4, CH4, LT4, [0, 1], [1, 2]), INVALID, b"the target root is not mapped"),
    ((0, CH4, LT4, [0], [0]), INVALID, b"trees of 1..64 joints (source 0, target 4)"),
    ((65, CH4, LT4, [0], [0]), UNSUPPORTED, b"trees of 1..64 joints (source 65, target 4)"),
    ((4, CH65, np.ones((65, 3), np.float32), [0], [0]), UNSUPPORTED, b"trees of 1..64 joints (source 4, target 65)"),
    ((4, np.array([0, 0, 1, 2]), LT4, [0], [0]), INVALID, b"joint 0 must be the root"),
    ((4, np.array([-1, 0, 3, 2]), LT4, [0], [0]), INVALID, b"parents[2]=3 is not < 2"),
])
def test_plan_rejections(args, status, msg):
    lib = _lib()
    assert _tables(*args) == status
    assert msg in lib.rtg_last_error(), lib.rtg_last_error()
    assert b"rtg_fit_targets_plan_tables" in lib.rtg_last_error()


def test_plan_create_and_launch_rejections_with_null_handles():
    lib = _lib()
    x, h = ctypes.c_void_p(64), ctypes.c_void_p()
    one = np.zeros(1, np.int32).ctypes.data_as(IP)
    assert lib.rtg_fit_targets_plan_create(None, None, one, one, 1, None, None, None, None) == INVALID
    assert b"rtg_fit_targets_plan_create: out is NULL" in lib.rtg_last_error()
    for src, tgt in ((None, x), (x, None), (None, None)):
        assert lib.rtg_fit_targets_plan_create(src, tgt, one, one, 1, None, None, None, ctypes.byref(h)) == INVALID
        assert b"rtg_fit_targets_plan_create: NULL topology" in lib.rtg_last_error()
        assert not h.value
    assert lib.rtg_fit_targets_plan_destroy(None) == 0
    assert lib.rtg_fit_targets_f32(None, x, 1, x, None) == INVALID
    assert b"rtg_fit_targets_f32: NULL plan" in lib.rtg_last_error()
    assert lib.rtg_fit_targets_f32(None, x, 0, x, None) == INVALID   # the handle is checked before B == 0 returns
    assert b"NULL plan" in lib.rtg_last_error()
    assert lib.rtg_fit_targets_f32(None, x, -1, x, None) == INVALID
    assert b"rtg_fit_targets_f32: B=-1 < 0" in lib.rtg_last_error()


class _Tree:
    def __init__(self, par, lt, names):
        self.parent_indices, self.local_translation, self.node_names = torch.as_tensor(par), torch.as_tensor(lt), names
        self.num_joints = len(par)


def test_python_entry_points_raise_rtg_error_without_a_gpu(monkeypatch):
    from rtg import _lib, ops
    from rtg.bridge import fit_targets_plan
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # the same test on a machine that has one
    from retarget.retarget_solver import VtrdynFullBodyFitRetargeter
    from robot_kinematics_model.hu_forward_model import HuForwardModel

    class Plan:   # what ops looks at before it asks for the device
        num_source_joints, num_target_joints, handle = 4, 4, None
    x = np.zeros((2, 4, 3), np.float32)
    with pytest.raises(_lib.RtgError):
        ops.fit_targets(Plan(), x)
    with pytest.raises(_lib.RtgError):
        fit_targets_plan((CH4, LT4), (CH4, LT4), [0], [0])
    tree = _Tree(CH4, LT4, list("abcd"))
    hu = HuForwardModel.__new__(HuForwardModel)   # its constructor already needs the device
    hu.num_joints, hu.node_names, hu.parent_indices, hu.sk_local_translation = 4, list("abcd"), CH4, LT4
    with pytest.raises(_lib.RtgError):
        hu.keypoint_targets(tree, {"a": "a"}, x)
    with pytest.raises(_lib.RtgError):
        hu.fit_mocap(tree, {"a": "a"}, x)

    class Zero:
        skeleton_tree = tree
    with pytest.raises(_lib.RtgError):
        VtrdynFullBodyFitRetargeter(Zero(), Zero(), {"a": "a"}).retarget_batch(x)


# ------------------------------------------------------------------ the host tables and limb_ratio
def _check_tables(Js, tp, tlt, sj, tj):
    from rtg import ops
    got, want = ops.fit_targets_tables(Js, tp, tlt, sj, tj), ref.tables(tp, tlt, sj, tj)
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k   # seg: bit for bit
    return got


def _check_ratio(sp, slt, tp, tlt, sj, tj, link):
    from rtg import ops
    got = ops.limb_ratio((sp, slt), (tp, tlt), (sj, tj), link)
    assert got == ref.limb_ratio(sp, slt, tp, tlt, sj, tj, link)
    return got


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_tables_and_limb_ratio_on_the_shipped_assets(case):
    s, t, sj, tj, c = ref.golden_mapping(case)
    (sp, slt), (tp, tlt) = _asset(s), _asset(t)
    got = _check_tables(len(sp), tp, tlt, sj, tj)
    names = c["target_names"]
    assert got["weight"].sum() == len(sj) and all(got["weight"][j] == 1 for j in tj)
    k = list(tj).index(names.index("left_ankle_link"))   # the ankle hangs from the knee, the knee from hip pitch
    assert names[tj[got["anchor"][k]]] == "left_knee_link"
    assert names[tj[got["anchor"][got["anchor"][k]]]] == "left_hip_pitch_link"
    for j in np.flatnonzero(tp == names.index("left_ankle_link")):   # an unmapped link under the ankle (Hu's toe) follows it
        assert got["weight"][j] == 0 and names[tj[got["src_of"][j]]] == "left_ankle_link"
    assert case != "vtrdyn_full_hu" or "left_toe_link" in names
    for link in ("left_ankle_link", "right_wrist_yaw_link"):
        r = _check_ratio(sp, slt, tp, tlt, sj, tj, names.index(link))
        assert 0.5 < r < 2.0   # a human-sized suit and a human-sized robot


@pytest.mark.parametrize("kind", SYNTHETIC)
def test_tables_and_limb_ratio_on_synthetic_trees(kind):
    sp, slt, tp, tlt, sj, tj = ref.synthetic(kind)
    got = _check_tables(len(sp), tp, tlt, sj, tj)
    if kind == "k1":   # only the root kept: every link copies it, nothing to rescale
        assert got["anchor"].tolist() == [-1] and not got["src_of"].any() and got["weight"].sum() == 1
        return
    if kind == "chain64_half":   # an odd link follows the even one before it; a segment spans two offsets
        assert got["src_of"].tolist() == [j // 2 for j in range(64)]
        G = ref.zero_pose_global(tp, tlt)
        assert np.array_equal(got["seg"][5], G[10] - G[8])
    if kind == "star60":
        assert all(a == list(tj).index(0) for k, a in enumerate(got["anchor"]) if tj[k] != 0)
    _check_ratio(sp, slt, tp, tlt, sj, tj, len(tp) - 1)


# ------------------------------------------------------------------ the restatement is the reference's rescale
def test_fma32_is_fmaf():
    libm = ctypes.CDLL("libm.so.6")
    libm.fmaf.restype, libm.fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    rng = np.random.default_rng(0)
    a, b, c = (rng.normal(size=4000).astype(np.float32) * np.float32(10.0) ** rng.integers(-25, 19, 4000)
               for _ in range(3))
    c[::3] = -(a * b)[::3]               # cancellation: the product's low half decides
    c[1::7] *= np.float32(2.0) ** -30    # a sum that needs more than 53 bits: the case round-to-odd is for
    special = np.array([0, -0.0, 1e-45, -1e-45, 1e-38, 3e38, -3e38, np.inf, -np.inf, np.nan, 1, 1 + 2 ** -23],
                       np.float32)
    a, b, c = (np.concatenate([v, np.resize(np.roll(special, i), 600)]) for i, v in enumerate((a, b, c)))
    want = np.array([libm.fmaf(*t) for t in zip(a.tolist(), b.tolist(), c.tolist())], np.float32)
    assert ref.same_bits(ref.fma32(a, b, c), want)


def test_restatement_is_the_reference_rescale():
    """tests/golden/motion_prep.npz holds the input and output of the reference's coord_transform +
    rescale_motion_to_standard_size on the VTRDyn zero pose (tools/make_golden.py): one tree, the identity mapping."""
    d = golden("motion_prep")
    par, lt = _asset("vtrdyn")
    ident = np.arange(len(par), dtype=np.int32)
    out = ref.fit_targets(par, lt, ident, ident, d["raw"], dir=[-1.0, -1.0, 1.0])
    assert np.isfinite(d["rescaled"]).all() and d["raw"].shape[0] == 64
    assert np.array_equal(out.view(np.uint32), d["rescaled"].view(np.uint32))
    perm = np.random.default_rng(0).permutation(len(par))   # the order the pairs are given in does not matter
    assert ref.same_bits(ref.fit_targets(par, lt, ident[perm], ident[perm], d["raw"], dir=[-1.0, -1.0, 1.0]), out)


# ------------------------------------------------------------------ what the feature is for
def test_rescaled_keypoints_fit_closer_than_raw_ones():
    """The float64 loop of tests/test_pose_fit_host.py on the recipe of fit_targets_ref.outcome_recipe (seed 1, the
    first one tried): 33-link Hu, 64 frames, a human with legs x 1.35, arms x 1.2, torso and neck x 1.25, the 15 links
    of the golden VTRDyn -> Hu mapping observed, 128 Adam steps at lr 0.02 with both root blocks fitted.  Measured:
    raw keypoints mean loss 0.2155, mean error to the truly posed robot 0.0608 m; limb-wise rescaled keypoints with
    the root translation x the leg-length ratio 0.7407: 0.00197 and 0.0091 m -- 109 times and 6.7 times lower."""
    x, o = ref.outcome_recipe(), ref.outcome_float64()
    print(f"leg-length ratio {x['ratio']:.4f}; raw: loss {o['raw'][0]:.4f}, error {o['raw'][1]:.4f} m; rescaled: loss "
          f"{o['rescaled'][0]:.5f}, error {o['rescaled'][1]:.4f} m; ratios {o['raw'][0] / o['rescaled'][0]:.1f}, "
          f"{o['raw'][1] / o['rescaled'][1]:.2f}")
    assert abs(x["ratio"] - 1 / 1.35) < 1e-6
    assert o["raw"][1] / o["rescaled"][1] >= 3
    assert o["raw"][0] / o["rescaled"][0] >= 20

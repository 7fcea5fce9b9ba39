"""CPU-only checks of ``retarget_to``: the test-side composition of oracle primitives (tests/retarget_to_ref.py)
reproduces the reference's recorded outputs (tests/golden/retarget_to.npz) bit for bit, the library's host plan tables
(rtg_retarget_plan_tables: the reduced trees, perm, src_of) agree with the fixture's names and with hand-made trees,
the drop-in's tree reduction leaves its tree alone, and the assertions / limits / no-GPU behaviour are as documented."""
import numpy as np
import pytest
import torch

import retarget_to_ref as ref
from retarget_to_ref import FIXTURE_CASES, bits, fixture, fixture_plan


def tables(sp, tp, sj, tj):
    from rtg.runtime import retarget_tables
    return {k: [int(x) for x in v] for k, v in retarget_tables(sp, tp, sj, tj).items()}


def check_tables(sp, tp, sj, tj):
    """The library's tables against the plain-Python ones; returns them."""
    got = tables(sp, tp, sj, tj)
    kept_s, sred, kept_t, tred, perm, src_of = ref.plan_tables(sp, tp, sj, tj)
    assert got == {"kept_src": kept_s, "src_reduced_parents": sred, "kept_tgt": kept_t, "tgt_reduced_parents": tred,
                   "perm": perm, "src_of": src_of}
    return got


# ------------------------------------------------------------------ the composition is the reference, bit for bit
@pytest.mark.parametrize("tag", FIXTURE_CASES)
def test_oracle_composition_reproduces_the_reference(tag):
    d, _ = fixture()
    plan, _ = fixture_plan(tag)
    rot, root = plan(d[f"{tag}_rot"], d[f"{tag}_root_t"], bool(d[f"{tag}_is_local"]))
    assert rot.shape == d[f"{tag}_out_rot"].shape and root.shape == d[f"{tag}_out_root_t"].shape
    np.testing.assert_array_equal(bits(rot), bits(d[f"{tag}_out_rot"]))
    np.testing.assert_array_equal(bits(root), bits(d[f"{tag}_out_root_t"]))


def test_fixture_covers_what_it_is_for():
    d, names = fixture()
    assert set(FIXTURE_CASES) <= set(names)
    for tag in FIXTURE_CASES:
        q, t = d[f"{tag}_rot"], d[f"{tag}_root_t"]
        assert q.shape[0] == 64 and t.shape == (64, 3)
        assert np.isnan(q[1]).any() and np.isinf(t[2]).any()                 # a NaN component, an inf root
        assert (np.abs(q[0]).sum(-1) == 0).any()                             # a zero quaternion
        assert np.isnan(d[f"{tag}_out_root_t"][2]).any() or np.isinf(d[f"{tag}_out_root_t"][2]).any()
        finite = np.isfinite(d[f"{tag}_out_rot"]).all(axis=(1, 2))
        assert finite[6:].all()                                             # the ordinary frames stay finite
    assert "neck_link" not in names["vtrdyn_hu_v5_local"]["mapping"].values()   # hu_v5 has no such link
    assert "neck_link" in names["vtrdyn_full_hu"]["mapping"].values()
    assert bool(d["vtrdyn_hu_v5_local_is_local"]) and not bool(d["vtrdyn_hu_v5_global_is_local"])


# ------------------------------------------------------------------ the host plan tables
@pytest.mark.parametrize("tag", FIXTURE_CASES)
def test_plan_tables_on_the_fixture_trees(tag):
    d, names = fixture()
    e = names[tag]
    s, t = ref.asset(e["source"]), ref.asset(e["target"])
    sj = [e["source_names"].index(a) for a in e["mapping"]]
    tj = [e["target_names"].index(b) for b in e["mapping"].values()]
    got = check_tables(s["parent_indices"], t["parent_indices"], sj, tj)
    assert [e["source_names"][j] for j in got["kept_src"]] == [n for n in e["source_names"] if n in e["mapping"]]
    if tag == names["drop"]["case"]:   # the reference's own reduced tree
        assert [e["source_names"][j] for j in got["kept_src"]] == names["drop"]["names"]
        assert got["src_reduced_parents"] == [int(p) for p in d["drop_parents"]]
    for k, j in enumerate(got["kept_tgt"]):   # perm: T_red's k-th joint is fed by the source joint mapped to it
        src_name = e["source_names"][got["kept_src"][got["perm"][k]]]
        assert e["mapping"][src_name] == e["target_names"][j]


CHAIN = [-1, 0, 1, 2, 3, 4]
STAR = [-1, 0, 0, 0, 0, 0]
BRANCHY = [-1, 0, 1, 1, 0, 4, 4, 2]


def test_plan_tables_on_hand_made_trees():
    # a chain with an unmapped interior joint and an unmapped leaf: 3 hangs from 1, joint 5 follows 4
    got = check_tables(CHAIN, CHAIN, [0, 1, 3, 4], [0, 1, 3, 4])
    assert got["src_reduced_parents"] == [-1, 0, 1, 2] and got["src_of"] == [0, 1, 1, 2, 3, 3]
    # a star: every kept leaf hangs from the root; unmapped leaves follow the root
    got = check_tables(STAR, STAR, [0, 2, 4], [0, 4, 2])
    assert got["src_reduced_parents"] == [-1, 0, 0] and got["perm"] == [0, 2, 1] and got["src_of"] == [0, 0, 1, 0, 2, 0]
    # K = 1: the roots only
    got = check_tables(BRANCHY, CHAIN, [0], [0])
    assert got["kept_src"] == [0] and got["src_of"] == [0] * 6 and got["perm"] == [0]
    # K = J, the identity and a crossed mapping between different trees
    got = check_tables(BRANCHY, BRANCHY, list(range(8)), list(range(8)))
    assert got["src_reduced_parents"] == BRANCHY and got["perm"] == list(range(8)) and got["src_of"] == list(range(8))
    check_tables(CHAIN, STAR, [0, 1, 2, 3, 4, 5], [0, 5, 4, 3, 2, 1])
    # an unmapped interior joint of a branching tree, the roots mapped to non-roots of each other
    got = check_tables(BRANCHY, BRANCHY, [0, 3, 7, 6], [5, 0, 7, 3])
    assert got["kept_src"] == [0, 3, 6, 7] and got["src_reduced_parents"] == [-1, 0, 0, 0]
    assert got["tgt_reduced_parents"] == [-1, 0, 0, 0] and got["src_of"] == [0, 0, 0, 1, 0, 2, 0, 3]


def test_bad_mappings_and_limits_are_rejected():
    from rtg import _lib
    with pytest.raises(_lib.RtgError, match="the root node cannot be dropped"):
        tables(CHAIN, CHAIN, [1, 2], [0, 1])
    with pytest.raises(_lib.RtgError, match="the root node cannot be dropped"):
        tables(CHAIN, CHAIN, [0, 2], [1, 2])
    with pytest.raises(_lib.RtgError, match="the joint mapping is not consistent with the skeleton trees"):
        tables(CHAIN, CHAIN, [0, 1, 2], [0, 3, 3])
    with pytest.raises(_lib.RtgError, match="out of range"):
        tables(CHAIN, CHAIN, [0, 6], [0, 1])
    with pytest.raises(_lib.RtgError, match="empty"):
        tables(CHAIN, CHAIN, [], [])
    big = [-1] + list(range(64))            # 65 joints: past the lane-group limit
    with pytest.raises(_lib.RtgError, match="at most|1\\.\\.64") as ei:
        tables(big, CHAIN, [0], [0])
    assert ei.value.status == 4             # RTG_ERR_UNSUPPORTED
    with pytest.raises(_lib.RtgError, match="1\\.\\.64"):
        tables(CHAIN, big, [0], [0])
    ok = [-1] + list(range(63))             # 64 joints: the limit itself is served
    assert tables(ok, ok, [0, 63], [0, 63])["src_of"] == [0] * 63 + [1]


def test_launch_entry_point_validates_before_device_work():
    import ctypes
    from rtg import _lib
    lib = _lib.lib()
    x = ctypes.c_void_p(64)   # never dereferenced: every call below fails validation
    assert lib.rtg_retarget_to_f32(None, x, x, 1, 1, x, x, None) == 1 and b"NULL plan" in lib.rtg_last_error()
    h = ctypes.c_void_p()
    assert lib.rtg_retarget_plan_create(None, None, None, None, 0, None, None, None, None, None, 1.0,
                                        ctypes.byref(h)) == 1
    assert b"NULL topology" in lib.rtg_last_error() and not h.value
    assert lib.rtg_retarget_plan_destroy(None) == 0
    assert lib.rtg_abi_version() == _lib.ABI_VERSION >= 6


# ------------------------------------------------------------------ the drop-in's host code
def _tree(names, parents, lt=None, quat=None):
    from poselib.poselib.skeleton.skeleton3d import SkeletonTree
    lt = np.arange(3 * len(names), dtype=np.float32).reshape(-1, 3) * 0.25 + 0.1 if lt is None else lt
    return SkeletonTree(list(names), torch.as_tensor(parents), torch.from_numpy(np.asarray(lt, np.float32)), quat)


def test_tree_reduction_matches_the_reference_and_leaves_the_tree_alone():
    d, names = fixture()
    e = names[names["drop"]["case"]]
    a = ref.asset(e["source"])
    tree = _tree(e["source_names"], a["parent_indices"], a["local_translation"])
    before = (tree.local_translation.clone(), tree.parent_indices.clone(), list(tree.node_names))
    red = tree.drop_nodes_by_names(names["drop"]["dropped"])
    assert list(red.node_names) == names["drop"]["names"]
    assert [int(p) for p in red.parent_indices] == [int(p) for p in d["drop_parents"]]
    kept = tree.keep_nodes_by_names(names["drop"]["names"])
    assert list(kept.node_names) == list(red.node_names)
    assert torch.equal(kept.local_translation, red.local_translation)
    assert torch.equal(tree.local_translation, before[0]) and torch.equal(tree.parent_indices, before[1])
    assert list(tree.node_names) == before[2]
    # the dropped links are summed node first, then up the chain, in float32 (:239-242)
    lt = a["local_translation"].astype(np.float32)
    par = [int(p) for p in a["parent_indices"]]
    for i, n in enumerate(red.node_names):
        j = e["source_names"].index(n)
        want, p = lt[j].copy(), par[j]
        while p != -1 and e["source_names"][p] in names["drop"]["dropped"]:
            want, p = want + lt[p], par[p]
        np.testing.assert_array_equal(red.local_translation[i].numpy(), want)
    # a pairwise table replaces the sums for every non-root joint
    J = len(par)
    pw = torch.arange(J * J * 3, dtype=torch.float32).reshape(J, J, 3)
    red2 = tree.drop_nodes_by_names(names["drop"]["dropped"], pw)
    for i, n in enumerate(red2.node_names):
        if i:
            p = e["source_names"].index(red2.node_names[int(red2.parent_indices[i])])
            assert torch.equal(red2.local_translation[i], pw[p, e["source_names"].index(n)])
    assert torch.equal(tree.local_translation, before[0])
    with pytest.raises(AssertionError, match="the root node cannot be dropped"):
        tree.drop_nodes_by_names([e["source_names"][0]])


def _state(tree, B=3):
    from poselib.poselib.skeleton.skeleton3d import SkeletonState
    q = np.tile(np.array([0, 0, 0, 1], np.float32), (B, len(tree), 1))
    return SkeletonState(torch.from_numpy(np.concatenate([q.reshape(B, -1), np.zeros((B, 3), np.float32)], -1)), tree, True)


def test_retarget_to_assertions_shape_rule_and_no_gpu():
    from rtg import _lib
    src = _tree("abcdef", CHAIN)
    tgt = _tree("ABCDEF", STAR)
    st = _state(src)
    tp_s, tp_t = _state(src, 1).tensor[0], _state(tgt, 1).tensor[0]
    args = (tp_s[:24].reshape(6, 4), tp_s[24:], tgt, tp_t[:24].reshape(6, 4), tp_t[24:], torch.tensor([0., 0, 0, 1]), 1.0)
    with pytest.raises(AssertionError, match="the joint mapping is not consistent with the skeleton trees"):
        st.retarget_to({"a": "A", "b": "B", "x": "C"}, *args)          # a source name the tree does not have
    with pytest.raises(AssertionError, match="the joint mapping is not consistent with the skeleton trees"):
        st.retarget_to({"a": "A", "b": "B", "c": "B"}, *args)          # two sources for one target
    with pytest.raises(AssertionError, match="the root node cannot be dropped"):
        st.retarget_to({"b": "A", "c": "B"}, *args)
    with pytest.raises(AssertionError, match="the root node cannot be dropped"):
        st.retarget_to({"a": "B", "c": "C"}, *args)
    from poselib.poselib.skeleton.skeleton3d import SkeletonState
    for shape in ((27,), (2, 3, 27)):                                  # no batch dimension, two of them
        odd = SkeletonState(torch.zeros(shape), src, True)
        with pytest.raises(ValueError, match="exactly one batch dimension"):
            odd.retarget_to({"a": "A"}, *args)
    with pytest.raises(AssertionError, match="doesn't support vectorized operations"):
        st.retarget_to_by_tpose({"a": "A"}, _state(src, 2), _state(tgt, 1), args[5], 1.0)
    if not torch.cuda.is_available():   # the product path: an RtgError, no CPU fallback
        with pytest.raises(_lib.RtgError):
            st.retarget_to({"a": "A", "c": "C"}, *args)
        from rtg import ops
        with pytest.raises(_lib.RtgError):
            ops.retarget_to(None, st.rotation, st.root_translation, True)

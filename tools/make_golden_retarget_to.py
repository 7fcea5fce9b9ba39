"""Generate ``tests/golden/retarget_to.npz`` / ``retarget_to_names.json``: the reference's ``SkeletonState.retarget_to``.

Build-container only (it imports the reference through ``tools/refharness.py``).  Five cases of 64 seeded frames:

  vtrdyn_hu_v5_local    VTRDyn-21 -> Hu v5 (31), local-state input    VTRDYN2HU_JOINT_MAPPING
  vtrdyn_hu_v5_global   the same frames handed over as a global state
  vtrdyn_full_hu        VTRDyn-59 -> Hu (33)                          VTRDYN2HU_JOINT_MAPPING
  noitom_hu_v5          Noitom-21 -> Hu v5                            NOITOM2HU_JOINT_MAPPING
  hu_v5_identity        Hu v5 -> Hu v5, every joint mapped to itself

The Hu mappings are Hu_v5.py's, filtered to the names both trees hold.  Frames 0-4 of every case are special: a zero
quaternion row, a NaN component, an inf root translation, a negated row, a row with w = -1.  The reference's
``drop_nodes_by_names`` adds into its own tree's translations, so every reference call gets a freshly built source tree.
Per case the file holds the inputs (the state's rotations and root translation as the state stores them), the t-poses,
R, s, and the output state's rotations and root translation; the mapping and the node names go to the JSON file.  For
``vtrdyn_full_hu`` it also holds ``SkeletonState.drop_nodes_by_names``' result: the reduced tree (names in the JSON;
parents; local translations in float32 and from a float64 run of the same code) and the reduced state's rotations.
Data only; fixed zip timestamps, so a rerun reproduces the file byte for byte.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import refharness as rh  # noqa: E402
from make_golden_grad import save_npz  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "retarget_to.npz")
OUT_NAMES = os.path.join(REPO, "tests", "golden", "retarget_to_names.json")
N = 64

CASES = (
    # tag, source asset, target asset, mapping name (None: identity), local-state input, seed
    ("vtrdyn_hu_v5_local", "vtrdyn", "hu_v5", "VTRDYN2HU_JOINT_MAPPING", True, 910),
    ("vtrdyn_hu_v5_global", "vtrdyn", "hu_v5", "VTRDYN2HU_JOINT_MAPPING", False, 910),
    ("vtrdyn_full_hu", "vtrdyn_full", "hu", "VTRDYN2HU_JOINT_MAPPING", True, 912),
    ("noitom_hu_v5", "noitom", "hu_v5", "NOITOM2HU_JOINT_MAPPING", True, 913),
    ("hu_v5_identity", "hu_v5", "hu_v5", None, True, 914),
)
DROP_CASE = "vtrdyn_full_hu"


def frames(rng, J):
    q = rng.normal(size=(N, J, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    q = q.astype(np.float32)
    t = rng.normal(0, 0.5, (N, 3)).astype(np.float32)
    j = J // 2
    q[0, j] = 0.0                       # a zero quaternion
    q[1, j, 1] = np.nan                 # a NaN component
    t[2, 0] = np.inf                    # an inf root translation
    q[3, j] = -q[3, j]                  # a negated row
    q[4, j] = (0.0, 0.0, 0.0, -1.0)     # w = -1
    q[5, 0] = -np.abs(q[5, 0])          # the root with w < 0
    return q, t


def main() -> None:
    import torch
    torch.set_num_threads(1)
    ref = rh.load_reference()
    sk = ref.skeleton3d
    out, names = {}, {}
    for tag, src, tgt, mapname, is_local, seed in CASES:
        def src_state():   # a fresh tree per reference call
            return rh.ref_skeleton_state(ref, src)
        s_tp, t_tp = src_state(), rh.ref_skeleton_state(ref, tgt)
        s_names, t_names = list(s_tp.skeleton_tree.node_names), list(t_tp.skeleton_tree.node_names)
        if mapname is None:
            mapping = {n: n for n in s_names}
        else:
            mapping = {a: b for a, b in getattr(ref.Hu_v5, mapname).items() if a in s_names and b in t_names}
        rng = np.random.default_rng(seed)
        q, t = frames(rng, len(s_names))
        Rq = rng.normal(size=4)
        Rq = (Rq / np.linalg.norm(Rq)).astype(np.float32)
        scale = float(rng.uniform(0.3, 1.7))
        state = sk.SkeletonState.from_rotation_and_root_translation(src_state().skeleton_tree, torch.from_numpy(q),
                                                                    torch.from_numpy(t), is_local=True)
        if not is_local:
            state = state.global_repr()
        res = state.retarget_to(mapping, s_tp.local_rotation.clone(), s_tp.root_translation.clone(),
                                t_tp.skeleton_tree, t_tp.local_rotation.clone(), t_tp.root_translation.clone(),
                                torch.from_numpy(Rq), scale)
        assert res.is_local
        out[f"{tag}_rot"] = state.rotation.numpy().copy()
        out[f"{tag}_root_t"] = state.root_translation.numpy().copy()
        out[f"{tag}_is_local"] = np.asarray(is_local)
        out[f"{tag}_src_tpose_rot"] = src_state().local_rotation.numpy().copy()
        out[f"{tag}_src_tpose_root_t"] = src_state().root_translation.numpy().copy()
        out[f"{tag}_tgt_tpose_rot"] = rh.ref_skeleton_state(ref, tgt).local_rotation.numpy().copy()
        out[f"{tag}_tgt_tpose_root_t"] = rh.ref_skeleton_state(ref, tgt).root_translation.numpy().copy()
        out[f"{tag}_R"] = Rq
        out[f"{tag}_scale"] = np.asarray(scale, np.float64)
        out[f"{tag}_out_rot"] = res.rotation.numpy().copy()
        out[f"{tag}_out_root_t"] = res.root_translation.numpy().copy()
        names[tag] = {"source": src, "target": tgt, "mapping": mapping, "source_names": s_names,
                      "target_names": t_names}
        if tag == DROP_CASE:
            drop = [n for n in s_names if n not in mapping]
            rng2 = np.random.default_rng(seed + 100)   # the average runs over frames: 64 frames without the special ones
            qf = rng2.normal(size=(N, len(s_names), 4))
            qf = (qf / np.linalg.norm(qf, axis=-1, keepdims=True)).astype(np.float32)
            tf = rng2.normal(0, 0.5, (N, 3)).astype(np.float32)
            for dt, sfx in ((torch.float32, "f32"), (torch.float64, "f64")):
                tree = src_state().skeleton_tree
                tree._local_translation = tree.local_translation.to(dt)
                st = sk.SkeletonState.from_rotation_and_root_translation(tree, torch.from_numpy(qf).to(dt),
                                                                         torch.from_numpy(tf).to(dt), is_local=True)
                red = st.drop_nodes_by_names(drop)
                out[f"drop_local_t_{sfx}"] = red.skeleton_tree.local_translation.numpy().copy()
                if dt == torch.float32:
                    out["drop_rot_in"] = qf
                    out["drop_root_t_in"] = tf
                    out["drop_parents"] = red.skeleton_tree.parent_indices.numpy().astype(np.int32)
                    out["drop_rot"] = red.rotation.numpy().copy()
                    out["drop_is_local"] = np.asarray(red.is_local)
                    names["drop"] = {"case": tag, "dropped": drop, "names": list(red.skeleton_tree.node_names)}
    save_npz(OUT, out)
    with open(OUT_NAMES, "w") as f:
        json.dump(names, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays) and {OUT_NAMES}")


if __name__ == "__main__":
    main()

"""The motion-velocity kernels (rtg_linear_velocity_f32, rtg_angular_velocity_f32: k_velocity_tile, k_gradient_dt,
k_angular_raw, k_gauss_nearest) on hostile input, bit for bit against the C oracle: the rotation and position sequences
of tests/kinematics_frames.py (static clips, antipodal flips, half turns, steps down to 1e-9, relative rotations whose
w sits on a table edge, products on, at the edge of and off the near-unit table, non-unit, tiny and huge rows, zero /
NaN / inf rows and elements; static, ramp, subnormal, overflowing and cancelling positions), one sequence per family in
a launch, through every tile shape of launch_velocity_tile / vel_tile_frames and the two-pass kernels, three filters and
ten frame times.  tests/test_kinematics_hostile_host.py anchors the oracle on these families to the reference's own
outputs and checks the oracle-only conditions (which rare paths the inputs reach).

Every comparison is on the raw bits, every NaN reading alike (retarget_to_ref.bits): +0.0 and -0.0 differ."""
import numpy as np
import pytest
import torch

import kinematics_frames as kf
from retarget_to_ref import bits

pytestmark = pytest.mark.gpu

# J -> frames per tile of the one-pass kernel at the reference's radius 8 (0: rows too wide, the two-pass kernels)
TILE_OF_J = {3: 64, 31: 64, 60: 32, 100: 16, 130: 0}
# the issue's frame times, then two of this file's: 3e38 makes every ordinary quotient subnormal (1e30 only dividends
# below 1.2e-8), the subnormal 1e-40 overflows every ordinary quotient (1e-30 only dividends above 3.4e8)
DTS = (1 / 30, 1 / 50, 1 / 120, 1.0, 3.0, 1e-3, 1e30, 1e-30, 3e38, 1e-40)
FILTERS = (("radius 8", 2.0), ("radius 4", 1.0), ("raw", None))
# (J, L, nseq per launch): every J with L = 130 and 8 sequences (blocks a multiple of 8: the XCD order); every L with
# J = 31, all families in one launch (19 and 9 sequences: never a multiple of 8) and one sequence alone
SHAPES = [(J, 130, 8) for J in TILE_OF_J] + [(31, L, 0) for L in (1, 2, 9, 17, 64, 65)]


def _vel(kind, x, dt, sigma):
    from rtg import ops
    fn = ops.motion_angular_velocity if kind == "ang" else ops.motion_velocity
    out = fn(x, dt) if sigma == 2.0 else (fn(x, dt, smooth=False) if sigma is None else fn(x, dt, sigma=sigma))
    return out.cpu().numpy()


def _oracle(kind, x, dt, sigma):
    import oracle as orc
    from rtg import ops
    w = None if sigma is None else ops.gaussian_taps(sigma)[0]
    with np.errstate(all="ignore"):
        return (orc.angular_velocity if kind == "ang" else orc.linear_velocity)(x, dt, w)


def _diff(got, want, names):
    """Names the sequences (families) that differ and the first few (sequence, frame, joint, component)."""
    bad = bits(got) != bits(want)
    if not bad.any():
        return ""
    at = np.argwhere(bad)
    seqs = sorted(set(at[:, 0].tolist())) if got.ndim == 4 else [0]
    return f"{int(bad.sum())} elements differ, in {[names[s] for s in seqs]}; first {at[:4].tolist()}: " \
           f"got {got[bad][:4]} want {want[bad][:4]}"


def _batches(kind, L, J, nseq):
    """[(names, (n, L, J, 3 | 4))]: every family once; nseq 8: launches of 8 sequences (the last padded with further
    smooth / random sequences); nseq 0: all families in one launch (positions: nine), then one sequence alone (L, J, .)."""
    fams = kf.ROT_FAMILIES if kind == "ang" else kf.POS_FAMILIES
    build = kf.rot_sequence if kind == "ang" else kf.pos_sequence
    names, seqs = list(fams), [build(f, L, J) for f in fams]
    pad = "smooth" if kind == "ang" else "random"
    if nseq == 0:
        if len(seqs) % 8 == 0:
            names.append(pad)
            seqs.append(build(pad, L, J, seed=1))
        return [(names, np.stack(seqs)), ([pad], build(pad, L, J, seed=2))]
    k = 0
    while len(seqs) % nseq:
        k += 1
        names.append(pad)
        seqs.append(build(pad, L, J, seed=k))
    return [(names[i:i + nseq], np.stack(seqs[i:i + nseq])) for i in range(0, len(seqs), nseq)]


@pytest.mark.parametrize("J,L,nseq", SHAPES)
def test_families_vs_oracle(gpu, J, L, nseq):
    """Every rotation and position family against the oracle: the reference's filter (radius 8, the constant-radius
    kernel), sigma 1 (radius 4, the generic-radius kernel) and raw; every frame time.  L = 1: angular only (np.gradient
    needs two frames; rtg_linear_velocity_f32 refuses one)."""
    from rtg import ops
    assert ops.gaussian_taps(2.0)[1] == 8 and ops.gaussian_taps(1.0)[1] == 4
    fails = []
    for kind in ("ang", "lin") if L > 1 else ("ang",):
        for names, x in _batches(kind, L, J, nseq):
            dev = torch.from_numpy(x).cuda()
            for fname, sigma in FILTERS:
                for dt in DTS:
                    msg = _diff(_vel(kind, dev, dt, sigma), _oracle(kind, x, dt, sigma), names)
                    if msg:
                        fails.append(f"{kind} {fname} dt={dt:g} nseq={x.shape[0] if x.ndim == 4 else 1}: {msg}")
    assert not fails, f"{len(fails)} launches off the oracle:\n" + "\n".join(fails[:12])


def test_tie_quotients(gpu):
    """Quotients by dt that are exact ties between two subnormal float32 values (kinematics_frames.midpoint_ramp,
    angular_tie_sequence): IEEE division rounds them to even; a product by the rounded reciprocal of dt rounds 30-45 %
    of them the other way (tests/test_kinematics_hostile_host.py), which is what the subnormal branch of the kernels'
    shared-reciprocal division is for.  Every filter, and radius 0 (sigma 0.1), whose output is the raw value itself."""
    cases = [("lin", kf.midpoint_ramp(130, 31, dt), dt) for dt in kf.TIE_DIVISORS[:3]]
    cases.append(("ang", kf.angular_tie_sequence(130, 31), kf.ANGULAR_TIE_DT))
    fails = []
    for kind, x, dt in cases:
        for fname, sigma in FILTERS + (("radius 0", 0.1),):
            msg = _diff(_vel(kind, torch.from_numpy(x).cuda(), dt, sigma), _oracle(kind, x, dt, sigma), ["ties"])
            if msg:
                fails.append(f"{kind} dt={dt:g} {fname}: {msg}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("J", sorted(TILE_OF_J))
def test_smoothed_and_raw_kernels_agree(gpu, J):
    """The raw launch's output, smoothed on the host by the oracle's filter (kinematics_frames.gauss_nearest), equals
    the smoothed launch's bits: the one-pass kernel's LDS values are the raw kernels' values, halo and edge replication
    included (J = 130: the two-pass kernels, trivially the same raw values)."""
    from rtg import ops
    for kind in ("ang", "lin"):
        for names, x in _batches(kind, 130, J, 8):
            dev = torch.from_numpy(x).cuda()
            for dt in (1 / 30, 1e30, 1e-30):
                raw = _vel(kind, dev, dt, None)
                for sigma in (2.0, 1.0):
                    msg = _diff(_vel(kind, dev, dt, sigma), kf.gauss_nearest(raw, ops.gaussian_taps(sigma)[0]), names)
                    assert not msg, f"{kind} J={J} dt={dt:g} sigma={sigma}: {msg}"


def _rare_rows(kind, x, rng):
    """x (nseq, L, J, .) smooth / random, float32, in place: exactly one (frame, joint) element of every 512 consecutive
    ones replaced by a rare one, at an offset that moves from group to group.  Returns the number placed."""
    nseq, L, J, _ = x.shape
    flat = x.reshape(nseq * L * J, -1)
    n = 0
    for b in range(len(flat) // 512):
        e = 512 * b + (b * 37 + 11) % 512
        t = (e // J) % L
        prev = flat[e - J] if t > 0 else flat[e + J]           # the same joint one frame earlier (later at frame 0)
        c = n % 12
        if kind == "lin":
            flat[e] = [prev, -prev, np.float32([0.0, -0.0, 0.0]), np.float32([1e-45, -1e-42, 1e-39]), prev * 0 + 3e38,
                       prev * 0 - 3e38, prev, prev, prev, prev, prev, prev][c]
            if c >= 6:
                flat[e, c % 3] = (np.nan, np.inf, -np.inf, 1e6, np.float32(1e-3), -0.0)[c - 6]
        elif c == 0:
            flat[e] = prev                                       # a static pair: the identity, acos(1), the clamp
        elif c == 1:
            flat[e] = -prev                                      # antipodal
        elif c == 2:
            flat[e] = np.nextafter(prev, np.float32(2.0))        # one ulp off the previous frame
        elif c in (3, 4, 5):
            flat[e] = kf._f32(flat[e].astype(np.float64) * kf.near_unit_factor((16, -17, 33)[c - 3]))
        elif c == 6:
            flat[e] = 0.0
        elif c in (7, 8):
            flat[e, n % 4] = (np.nan, np.inf)[c - 7]
        elif c in (9, 10):
            flat[e] = kf._f32(flat[e].astype(np.float64) * (1e-40, 1e18)[c - 9])
        else:
            flat[e] = kf._f32(kf.qmul(np.append(kf._unit3(rng), 0.0), prev.astype(np.float64)))   # a half turn
        n += 1
    return n


@pytest.mark.parametrize("J", [31, 100])
def test_one_rare_element_per_batch(gpu, J):
    """A smooth motion (random positions) in which exactly one (frame, joint) element of every 512 is rare -- equal to,
    opposite to, one ulp or a half turn from its neighbour in time, a norm at the table's edge or off it, zero, NaN, inf,
    tiny, huge -- at a place in the 256-thread block that moves from block to block: every output equals the oracle, and
    every output the oracle leaves as in the clean motion keeps the clean launch's bits."""
    rng = np.random.default_rng(J)
    for kind in ("ang", "lin"):
        build = kf.rot_sequence if kind == "ang" else kf.pos_sequence
        clean = np.stack([build("smooth" if kind == "ang" else "random", 130, J, seed=s) for s in range(8)])
        dirty = clean.copy()
        n = _rare_rows(kind, dirty, rng)
        assert n == 8 * 130 * J // 512
        same_in = (bits(dirty) == bits(clean)).all(axis=-1)
        assert (~same_in).sum() >= n - n // 12 - 1             # the elements differ from the clean motion's
        for fname, sigma in FILTERS:
            for dt in (1 / 30, 1e30):
                want0, want1 = _oracle(kind, clean, dt, sigma), _oracle(kind, dirty, dt, sigma)
                got0, got1 = (_vel(kind, torch.from_numpy(a).cuda(), dt, sigma) for a in (clean, dirty))
                names = [f"sequence {s}" for s in range(8)]
                msg = _diff(got1, want1, names)
                assert not msg, f"{kind} {fname} dt={dt:g}: {msg}"
                keep = bits(want1) == bits(want0)
                assert 0.2 < keep.mean() < 1.0
                assert (bits(got1)[keep] == bits(got0)[keep]).all(), f"{kind} {fname} dt={dt:g}: a clean element moved"


@pytest.mark.parametrize("J", [31, 60, 100])
def test_single_bad_elements_are_isolated(gpu, J):
    """One NaN element, then one zero row, at frames 0, 1, L - 2, L - 1 and on both sides of every boundary of this
    shape's tile (64 / 32 / 16 frames), in the middle one of three sequences: every output the oracle leaves unchanged
    keeps the clean launch's bits (the other sequences and the tiles out of the filter's reach), every output it
    changes equals the oracle, and a second launch gives the same bits."""
    L, T = 130, TILE_OF_J[J]
    for kind in ("ang", "lin"):
        build = kf.rot_sequence if kind == "ang" else kf.pos_sequence
        clean = np.stack([build("smooth" if kind == "ang" else "random", L, J, seed=10 + s) for s in range(3)])
        for sigma in (2.0, None):
            want0 = _oracle(kind, clean, 1 / 30, sigma)
            got0 = _vel(kind, torch.from_numpy(clean).cuda(), 1 / 30, sigma)
            assert not _diff(got0, want0, ["a", "b", "c"])
            for bad in ("nan", "zero_row"):
                for i, t in enumerate(kf.placements(L, (T,))):
                    dirty = clean.copy()
                    kf.set_single(dirty[1], bad, t, (5 * i + 2) % J)
                    dev = torch.from_numpy(dirty).cuda()
                    want1 = _oracle(kind, dirty, 1 / 30, sigma)
                    got1, got2 = _vel(kind, dev, 1 / 30, sigma), _vel(kind, dev, 1 / 30, sigma)
                    tag = f"{kind} J={J} sigma={sigma} {bad} at frame {t}"
                    assert (bits(got1) == bits(got2)).all(), tag + ": two launches differ"
                    changed = bits(want1) != bits(want0)
                    assert changed.any() and not changed[[0, 2]].any(), tag
                    assert (bits(got1)[~changed] == bits(got0)[~changed]).all(), tag + ": an untouched output moved"
                    assert (bits(got1)[changed] == bits(want1)[changed]).all(), tag + ": off the oracle"


@pytest.mark.parametrize("family", ["static", "antipodal"])
def test_drop_in_motion_of_a_static_and_an_antipodal_state(gpu, family):
    """SkeletonMotion.from_skeleton_state on a Hu v5 state held on the device whose global rotations are a static clip
    (runs of identical frames, rows with -0.0 components) or flip sign from frame to frame: the velocity columns equal
    the oracle's velocities of the state's own global translations and rotations, bit for bit."""
    from poselib.poselib.skeleton.skeleton3d import SkeletonMotion
    from test_gpu_retarget_to import asset_tree, state_of
    tree = asset_tree("hu_v5")
    L, J = 40, tree.num_joints
    root = kf.pos_sequence("static", L, 1)[:, 0]
    st = state_of(tree, kf.rot_sequence(family, L, J), root, False, "cuda")
    for fps in (30, 120):
        mo = SkeletonMotion.from_skeleton_state(st, fps)
        assert mo.tensor.is_cuda and mo.tensor.shape == (L, J * 10 + 3)
        gp, gr = st.global_translation.cpu().numpy(), st.global_rotation.cpu().numpy()
        lin, ang = _oracle("lin", gp, 1 / fps, 2.0), _oracle("ang", gr, 1 / fps, 2.0)
        np.testing.assert_array_equal(bits(mo.global_velocity.cpu().numpy()), bits(lin))
        np.testing.assert_array_equal(bits(mo.global_angular_velocity.cpu().numpy()), bits(ang))
        raw = _oracle("ang", gr, 1 / fps, None)                  # the clip is what it is meant to be: still pairs
        assert (raw[:-1] == 0).all(axis=-1).mean() > (0.5 if family == "static" else 0.1)

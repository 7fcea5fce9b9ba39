"""Round 18's instruction cuts in the FULL_BODY_POS side kernel (k_solve_sides, reached only above RTG_LATENCY_MAX_B)
and in the kernels that share its fits, bit for bit against the oracle: one residual correction per fdiv_n quotient,
the exp-map read-out's unscaled square root, and store_dof_rows' carried (row, column).

B = RTG_LATENCY_MAX_B + 1 and + 65 in both layouts: a ragged last tile, one live row, and one live tile in the last
block.  The batch repeats a pool of 448 distinct frames (seven 64-frame waves, the oracle runs once on the pool), tile
by tile, with the first tile, the last whole tile and the lone row of the last tile chosen per B:

  wave 0  rtg.synth frames whose wrist fits are sweep_loop_cases' 2x2-block cases, lane by lane alternating between
          the split at E(1) (block (2, 3)) and the deflation at E(2) (block (1, 2));
  wave 1  the same with every lane a block (2, 3), wave 2 with every lane a block (1, 2) (whole waves);
  wave 3  rtg.synth frames with test_gpu_fit_division's scaled / near-diagonal / near-rank-1 / zero-line / denormal
          fits at lanes 0, 31, 32 and 63 and, over the families' variants, at lanes 7 .. 62, and the zero pose itself
          (identity arms: the arm chains' read-outs have w = 1 or one of the two floats below it, so 1 - w w is 0
          or 2^-24 .. 2^-22; the wrists' Euler links are small angles, w within 3e-5 of 1) at lanes 1 .. 6, plain,
          translated and scaled by powers of two -- asserted from the oracle's link quaternions;
  wave 4  rtg.synth frames with a frame the reference raises on (a NaN point) in rows 0 and 63;
  wave 5  all three fits nearly rank 1 in every lane: collinear points plus noise of 2^-52 .. 2^-62, which puts
          SLARTG's f and g between its own rtmin and the division window (the branch that redoes the common case
          with fdiv and cr_sqrt, whose f f + g g is below 2^-96);
  wave 6  the read-out's w forced through frames (_forced_w): the zero pose with each forearm turned about its elbow by
          phi.  About z that turn is the shoulder-yaw link's whole rotation (links 14 / 23, the arm chain), about x the
          wrist's Euler X link's (16 / 25), and the link's w is cos(phi / 2) as the kernel and the oracle round it.
          Found by a search with the oracle, not assumed: w = 0.25 exactly (the angle table's first entry) and the
          nearest w the link can take on either side of it, w = 1 - k 2^-24 for k = 0 .. 4 (1 and its float neighbours;
          the mask sin_theta > 1e-5 is false for w = 1 alone), and the smallest w there is, 4.37e-8 at phi = pi.

What w cannot be, so that no frame forces it.  Every link quaternion is {axis sin(a / 2), cos(a / 2)} of an f32 angle
a, normalised with its sign flipped where w < 0.  (1) w < 0, so w = -1, and -0 never reach the read-out: the flip
makes w >= 0, and a cosine is never -0.  (2) |w| > 1 cannot come out of the normalisation: w / |q| with |q| >= |w|
rounds to at most 1.  (3) w = 0 exactly needs cos(a / 2) = 0, which no f32 a / 2 gives (cos(RN(pi / 2)) = -4.37e-8).
(4) The float neighbours of 0.25 proper: a / 2 near acos(0.25) has an f32 spacing of 1.2e-7 and d cos = 0.97 d(a / 2),
so the w a link can take there are 4 to 8 codes apart; the search takes the nearest on each side (asserted within 16
codes).  tools/check_fdiv1 [R] covers every w for the square root itself; these frames run exp_dof_word_part /
exp_dof_tab / exp_dof_exact with the table edge and the mask in the kernels.

B = MAX + 1 ends in wave 3 as the last whole tile and a raising frame alone in the one-row tile; B = MAX + 65 ends in
wave 4 (raising frames in rows 0 and 63 of the last whole tile) and wave 0's lane 0 alone.  A poisoned row must equal
the oracle's (NaNs compare as NaN), and its neighbours must be untouched.

The same fits go through rtg_cal_joint_quat_f32 with 3 and 5 points in launches of 64, 65 and 130 (k_cal_joint_quat
and the small-batch kernels share la_bdsqr3), together with the exact 2x2-block bidiagonals (3 points, Z = I).

Mutants these fail on are listed in profiles/r18/mutants.txt."""
import numpy as np
import pytest
import torch

from conftest import golden
import sweep_loop_cases as slc
import test_gpu_fit_division as tfd

NWAVES = 7
POOL = 64 * NWAVES
SPECIAL_LANES = (0, 31, 32, 63)
FAMS = ["scaled", "near_diag", "near_rank1", "zero_line", "denormal"]


def _bits(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def _block_cases():
    """Index-order bidiagonals that end in one 2x2 block: (split at E(1): block (2, 3), deflation: block (1, 2))."""
    split, defl = [], []
    for lab, c in slc.index_cases():
        t = slc.thresh(*c)
        if lab.startswith("e1 about") and abs(c[3]) <= t < abs(c[4]):
            split.append(c)
        if lab.startswith("e2 about") and abs(c[4]) <= t < abs(c[3]):
            defl.append(c)
    assert len(split) >= 8 and len(defl) >= 8
    return split, defl


def _wrist_points(Zh, c):
    """Five hand points whose A = M^T Z is (up to rounding) the upper bidiagonal c = (d1, d2, d3, e1, e2)."""
    d1, d2, d3, e1, e2 = (float(v) for v in c)
    T = np.array([[d1, e1, 0.0], [0.0, d2, e2], [0.0, 0.0, d3]])
    return (np.linalg.pinv(Zh.astype(np.float64)).T @ T.T).astype(np.float32)


W_LINKS = ((2, 14, 23), (0, 16, 25))               # (axis of the elbow turn, left link, right link)
QUARTER = 0x3E800000                              # bits of 0.25f, the angle table's first entry


def _bent(zg, axis, phis):
    """The zero pose with both forearms (and hands) turned by phi about `axis` through the elbow, as solver inputs."""
    from rtg import synth
    a = np.eye(3)[axis]
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    out = np.repeat(zg.astype(np.float64)[None], len(phis), axis=0)
    for n, phi in enumerate(phis):
        R = np.eye(3) + np.sin(phi) * K + (1 - np.cos(phi)) * (K @ K)
        for pivot, moved in ((13, slice(14, 34)), (38, slice(39, 59))):
            out[n, moved] = (out[n, moved] - out[n, pivot]) @ R.T + out[n, pivot]
    p = out.astype(np.float32)
    return [np.ascontiguousarray(p[:, k]) for k in (synth.FULL_TO_BODY, synth.LH_SLICE, synth.RH_SLICE)]


def _forced_w(zl, zg):
    """[(phi, axis, link, what)] found with the oracle: for each link of W_LINKS the turn that gives w = 0.25 or the
    nearest w on either side, w = 1 - k 2^-24, and the smallest w (phi = pi)."""
    import oracle as orc

    def w_of(axis, phis):
        dof, lr, _ = orc.full_body_pos(zl, zg, *_bent(zg, axis, phis), True)
        assert (orc.frame_status(dof) == 0).all()
        return lr[:, :, 3]
    out = []
    for axis, *links in W_LINKS:
        coarse = np.linspace(-3.0, 3.0, 241)
        wc = w_of(axis, coarse)
        wpi = w_of(axis, np.array([np.pi]))
        for link in links:
            k = int(np.nonzero((wc[:-1, link] - 0.25) * (wc[1:, link] - 0.25) <= 0)[0][0])   # a crossing of 0.25
            lo, hi = coarse[k], coarse[k + 1]
            up = wc[k + 1, link] > wc[k, link]
            for _ in range(40):
                mid = 0.5 * (lo + hi)
                if (w_of(axis, np.array([mid]))[0, link] > 0.25) == up:
                    hi = mid
                else:
                    lo = mid
            fine = 0.5 * (lo + hi) + np.linspace(-3e-6, 3e-6, 601)
            code = w_of(axis, fine)[:, link].view(np.int32).astype(np.int64) - QUARTER
            below, above = code[code < 0].max(), code[code > 0].min()
            assert -16 <= below and above <= 16, (axis, link, below, above)
            for c in (below, 0, above):
                if (code == c).any():
                    out.append((float(fine[np.nonzero(code == c)[0][0]]), axis, link, f"w = 0.25 {int(c):+d} codes"))
            # w = 1: at the turn where the link's own angle passes through zero (0 for the arm chain; the wrist's Euler
            # X angle of the zero pose is not zero), then the turns beside it
            grid = np.linspace(-0.05, 0.05, 2001)
            top = grid[int(np.argmax(w_of(axis, grid)[:, link]))]
            near1 = top + np.linspace(0.0, 4e-3, 401)   # argmax is the left end of the plateau w = 1
            c1 = w_of(axis, near1)[:, link].view(np.int32).astype(np.int64) - 0x3F800000
            for kk in range(5):
                assert (c1 == -kk).any(), (axis, link, kk, c1)
                out.append((float(near1[np.nonzero(c1 == -kk)[0][0]]), axis, link, f"w = 1 - {kk} 2^-24"))
            if 0 < wpi[0, link] < 1e-6:
                out.append((float(np.pi), axis, link, "the smallest w"))
    return out


@pytest.fixture(scope="module")
def pool():
    import oracle as orc
    from rtg import synth
    zp = golden("zero_pose")
    zl, zg = zp["vtrdyn_full_local_t"], zp["vtrdyn_full_global_t"]
    body, lh, rh = (np.ascontiguousarray(a) for a in synth.synth_full_body_inputs(POOL, seed=1818))
    Zt, Zl, Zr = zl[list(tfd.TORSO_Z)], zl[list(tfd.LEFT_Z)], zl[list(tfd.RIGHT_Z)]
    split, defl = _block_cases()
    for i in range(3 * 64):                       # waves 0-2: the 2x2 blocks
        w, lane = divmod(i, 64)
        p1 = (lane % 2 == 0) if w == 0 else (w == 1)
        for s, (h, Zh) in enumerate(((lh, Zl), (rh, Zr))):
            cs = split if p1 else defl
            h[i, 0] = 0.0
            h[i, tfd.WRIST_JOINTS, :] = _wrist_points(Zh, cs[(i + 3 * s) % len(cs)])
    rng = np.random.default_rng(1801)
    for k, lane in enumerate(SPECIAL_LANES):      # wave 3: scaled / degenerate fits
        i = 3 * 64 + lane
        fam = FAMS[k % len(FAMS)]
        body[i, 10] = 0.0
        body[i, tfd.TORSO_JOINTS, :] = tfd._family_points(fam, Zt, 7 + k, rng)
        for j, (h, Zh) in enumerate(((lh, Zl), (rh, Zr))):
            h[i, 0] = 0.0
            h[i, tfd.WRIST_JOINTS, :] = tfd._family_points(FAMS[(k + 1 + j) % len(FAMS)], Zh, 11 + 5 * k + j, rng)
    for lane in range(7, 63):                     # wave 3, the lanes between: every family over its variants (near-rank-1
        if lane in SPECIAL_LANES:                 # noise of 2^-15 .. 2^-75 puts SLARTG's f and g below the division window)
            continue
        i, fam, v = 3 * 64 + lane, FAMS[lane % len(FAMS)], 3 * lane + 5
        body[i, 10] = 0.0
        body[i, tfd.TORSO_JOINTS, :] = tfd._family_points(fam, Zt, v, rng)
        for j, (h, Zh) in enumerate(((lh, Zl), (rh, Zr))):
            h[i, 0] = 0.0
            h[i, tfd.WRIST_JOINTS, :] = tfd._family_points(fam, Zh, v + 15 * (j + 1), rng)
    zpose = zg.astype(np.float32)                 # wave 3, lanes 1-6: the zero pose
    zb, zlh, zrh = zpose[synth.FULL_TO_BODY], zpose[synth.LH_SLICE], zpose[synth.RH_SLICE]
    shifts = [np.zeros(3, np.float32), np.array([0.5, -0.25, 1.0], np.float32), np.array([3.0, 7.0, -5.0], np.float32)]
    for k in range(6):
        i = 3 * 64 + 1 + k
        sc, sh = np.float32(2.0 ** (0, 0, 0, 3, -4, -9)[k]), shifts[k % 3]
        body[i], lh[i], rh[i] = zb * sc + sh, zlh * sc + sh, zrh * sc + sh
    tiny = [v for v in range(0, 1400, 3) if 22 <= v % 40 <= 32]   # near_rank1's collinear variant, noise 2^-(30 + v % 40)
    for lane in range(64):                        # wave 5
        i = 5 * 64 + lane
        body[i, 10] = 0.0
        body[i, tfd.TORSO_JOINTS, :] = tfd._family_points("near_rank1", Zt, tiny[(3 * lane) % len(tiny)], rng)
        for j, (h, Zh) in enumerate(((lh, Zl), (rh, Zr))):
            h[i, 0] = 0.0
            h[i, tfd.WRIST_JOINTS, :] = tfd._family_points("near_rank1", Zh, tiny[(3 * lane + 1 + j) % len(tiny)], rng)
    forced = _forced_w(zl, zg)                    # wave 6
    assert len(forced) <= 64
    for lane, (phi, axis, link, what) in enumerate(forced):
        i = 6 * 64 + lane
        body[i], lh[i], rh[i] = (a[0] for a in _bent(zg, axis, [phi]))
    for lane in (0, 63):                          # wave 4: frames the reference raises on
        body[4 * 64 + lane, 17, lane % 3] = np.nan
    lh[4 * 64 + 63, 2, 1] = np.nan
    odof, olr, obr = orc.full_body_pos(zl, zg, body, lh, rh, True)
    status = orc.frame_status(odof)
    assert (status[[4 * 64, 4 * 64 + 63]] != 0).all() and (np.delete(status, [4 * 64, 4 * 64 + 63]) == 0).all()
    assert np.isfinite(np.delete(odof, [4 * 64, 4 * 64 + 63], axis=0)).all()
    return dict(ins=(body, lh, rh), ref=(odof, olr, obr), status=status, Z=(Zt, Zl, Zr), forced=forced)


def _index(B):
    """Pool index of every frame of a batch of B = 64 T + 1 frames."""
    T = B // 64
    assert B == 64 * T + 1 and T >= 8
    waves = np.array([(0, 3, 4, 1, 2, 5, 6)[t % NWAVES] for t in range(T)])
    waves[0] = 0
    lone_is_raising = T % 2 == 0                  # MAX + 1: T even; MAX + 65: T odd
    waves[T - 1] = 3 if lone_is_raising else 4
    idx = (waves[:, None] * 64 + np.arange(64)[None, :]).reshape(-1)
    return np.concatenate([idx, [4 * 64 if lone_is_raising else 0]])


def test_pool_and_index_cover_what_they_claim(pool):
    """On the CPU: the two batches end as the module's text says, and the oracle's 2x2-block fits are finite."""
    for T, lone in ((768, 4 * 64), (769, 0)):
        idx = _index(64 * T + 1)
        assert idx[-1] == lone and (idx[:64] == np.arange(64)).all()
        assert (idx[64 * (T - 1):64 * T] // 64 == (3 if T % 2 == 0 else 4)).all()
        assert set(idx // 64) == set(range(NWAVES))
    assert pool["status"][4 * 64] != 0 and pool["status"][0] == 0
    # the zero-pose frames: every read-out link (12 .. 18, 21 .. 27) has w = 1 or one of its two neighbours below
    olr = pool["ref"][1]
    # (the arm chains'; the wrists' Euler links of the zero pose are small angles, not zero: w within 3e-5 of 1)
    arm, wrist = [12, 13, 14, 15, 21, 22, 23, 24], [16, 17, 18, 25, 26, 27]
    wz = olr[3 * 64 + 1:3 * 64 + 7][:, arm, 3]
    assert np.isin(wz, np.float32([1.0, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -23])).all(), wz
    assert (wz == 1.0).any()
    ww = olr[3 * 64 + 1:3 * 64 + 7][:, wrist, 3]
    assert (ww > 1.0 - 3e-5).all() and (ww <= 1.0).all(), ww
    # the forced read-outs: the pool's own oracle run gives each frame's link the w the search found
    seen = set()
    for lane, (phi, axis, link, what) in enumerate(pool["forced"]):
        w = olr[6 * 64 + lane, link, 3]
        if what.startswith("w = 0.25"):
            assert int(w.view(np.int32)) - QUARTER == int(what.split()[3]), (what, link, w)
        elif what.startswith("w = 1 -"):
            assert w == np.float32(1.0 - int(what.split()[4]) * 2.0 ** -24), (what, link, w)
        else:
            assert 0 < w < 1e-6, (what, link, w)
        seen.add((link, what.split(" codes")[0] if "codes" not in what else ("0.25" if "+0" in what else "beside 0.25")))
    for _, *lk in W_LINKS:
        for link in lk:
            assert (link, "beside 0.25") in seen and all((link, f"w = 1 - {k} 2^-24") in seen for k in range(5)), link
    assert any(what == "w = 0.25 +0 codes" for _, _, _, what in pool["forced"])        # the table's first entry itself
    assert any(what == "the smallest w" for _, _, _, what in pool["forced"])


def _solver():
    from rtg import _lib, assets
    from rtg.runtime import Solver
    zp = golden("zero_pose")
    return Solver(_lib.SOLVER_FULL_BODY_POS, zp["vtrdyn_full_local_t"], zp["vtrdyn_full_global_t"],
                  assets.parents("vtrdyn_full"), True)


def _run(S, pool, idx, layout):
    dev = [torch.from_numpy(np.ascontiguousarray(a[idx])).cuda() for a in pool["ins"]]
    if layout == "soa":
        dev = [t.permute(1, 2, 0).contiguous() for t in dev]
    dof, lr, br = S.retarget(dev, want_local_rot=True, want_body_rot=True, layout=layout)
    return dof, lr, br


def _compare(pool, idx, outs, tag):
    from rtg.runtime import frame_status
    dof, lr, br = outs
    np.testing.assert_array_equal(frame_status(dof).cpu().numpy(), pool["status"][idx], err_msg=f"{tag}: status")
    for name, got, ref in (("dof", dof, pool["ref"][0]), ("local_rot", lr, pool["ref"][1]), ("body_rot", br, pool["ref"][2])):
        bad = np.nonzero((_bits(got.cpu().numpy()) != _bits(ref[idx])).reshape(len(idx), -1).any(axis=1))[0]
        assert bad.size == 0, (tag, name, bad.size, bad[:8], idx[bad[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("extra", [1, 65])
def test_side_kernel_vs_oracle(gpu, pool, layout, extra):
    from rtg import _lib
    B = _lib.build_info()["knobs"]["RTG_LATENCY_MAX_B"] + extra
    idx = _index(B)
    _compare(pool, idx, _run(_solver(), pool, idx, layout), f"B={B} {layout}")


@pytest.mark.gpu
def test_two_solvers_one_destroyed(gpu, pool):
    """Each solver owns its device tables: destroying one leaves the other's results what they were."""
    from rtg import _lib
    idx = _index(_lib.build_info()["knobs"]["RTG_LATENCY_MAX_B"] + 1)
    S1, S2 = _solver(), _solver()
    a = [t.cpu().numpy() for t in _run(S1, pool, idx, "soa")]
    b = [t.cpu().numpy() for t in _run(S2, pool, idx, "soa")]
    del S2
    torch.cuda.synchronize()
    S3 = _solver()                                # a new solver may take the freed memory
    outs = _run(S1, pool, idx, "soa")
    _compare(pool, idx, outs, "after destroying the other solver")
    for x, y, z in zip(a, b, outs):
        np.testing.assert_array_equal(_bits(x), _bits(y))
        np.testing.assert_array_equal(_bits(x), _bits(z.cpu().numpy()))
    del S3


@pytest.fixture(scope="module")
def fits(pool):
    """(Z, M, oracle) for cal_joint_quat: 3 points -- the exact 2x2-block bidiagonals alternating lane by lane, then in
    whole waves, then the pool's torso fits; 5 points -- the pool's left and right wrist fits."""
    import oracle as orc
    body, lh, rh = pool["ins"]
    Zt, Zl, Zr = pool["Z"]
    split, defl = _block_cases()
    alt = [(split if i % 2 == 0 else defl)[(i // 2) % 8] for i in range(64)]
    de = np.array(alt + [split[i % len(split)] for i in range(64)] + [defl[i % len(defl)] for i in range(64)], np.float32)
    Zb, Mb = slc.bidiag_points(de)
    Mt = body[:, tfd.TORSO_JOINTS, :] - body[:, 10:11, :]
    Z3 = np.concatenate([Zb, np.broadcast_to(Zt, (POOL, 3, 3))]).astype(np.float32)
    M3 = np.concatenate([Mb, Mt]).astype(np.float32)
    M5 = np.concatenate([h[:, tfd.WRIST_JOINTS, :] - h[:, 0:1, :] for h in (lh, rh)]).astype(np.float32)
    Z5 = np.concatenate([np.broadcast_to(Z, (POOL, 5, 3)) for Z in (Zl, Zr)]).astype(np.float32)
    return {3: (Z3, M3, orc.cal_joint_quat(Z3, M3)), 5: (Z5, M5, orc.cal_joint_quat(Z5, M5))}


@pytest.mark.gpu
@pytest.mark.parametrize("B", [64, 65, 130])
@pytest.mark.parametrize("npts", [3, 5])
def test_cal_joint_quat_vs_oracle(gpu, fits, npts, B):
    from rtg import ops
    Z, M, o = fits[npts]
    for s in range(0, len(Z), B):
        g = ops.cal_joint_quat(np.ascontiguousarray(Z[s:s + B]), np.ascontiguousarray(M[s:s + B])).cpu().numpy()
        bad = np.nonzero((_bits(g) != _bits(o[s:s + B])).any(axis=1))[0] + s
        assert bad.size == 0, (npts, B, bad.size, bad[:8])

"""Round 22's single IEEE quotients through the one-correction sequence (fdiv1, csrc/rtg_math.cuh): the reflector's
test (la_larfg), the bidiagonal's test per SBDSQR pass and at its entry (la_bdsqr3_pass, la_bdsqr3_entry), the constant
denominators sqrt(3) and 5, and the exp-map read-out's numerator test.  Everything is compared bit for bit, NaN equal
to NaN (tests/test_gpu_torso_fit.py's rule).

1.  tools/check_fdiv1 `single` on the device (built with the library's flags): fdiv1 behind its guard against a / b
    over every mantissa of the denominator in region [N]'s lowest and highest binades, in [1, 2) and one binade outside
    either end, under numerators at both numerator edges, one binade outside them, +-0, denormal, +-inf and NaN; the
    constant denominators over every f32 numerator; and each converted site against its a / b form on hashed operands
    scaled inside, on and outside the edges of its test.  Zero mismatches; every guard's verdict equals the one the
    tool works out from the bit patterns, so nothing outside a region runs bare.  The gripper's a / C.orig is not
    converted, so there are two constants, not three.

2.  Through the library against the C oracle: rtg_cal_joint_quat_f32 with 3 and 5 points and the FULL_BODY_POS solver
    at B = 1, 2, 65, RTG_LATENCY_MAX_B + 1 and + 65, both layouts, both gripper modes.  The frames are
    tests/test_gpu_fit_division.py's, aimed at the new tests.  SGESDD rescales the fitted matrix into [2^-40, 2^40],
    so the UPPER edges (2^45, 2^46) cannot be reached through the library -- the tool's site checks drive them -- and
    the lower ones are reached by small singular values under an ordinary norm:
      low_state   near-rank-1 and near-diagonal fits times 2^k, the small values placed one binade inside, on and
                  outside 2^-46 (the state's and the reflector's edge) and 2^-76 (the numerator edge of mu and sminoa);
      tiny        tiny mu and tiny e against an ordinary state (noise 2^-10 .. 2^-75 under norms 2^-36 .. 2^36);
      mixed       one wave whose lanes alternate between ordinary fits and low_state ones: in- and out-of-window
                  states in one pass;
      zeros       exactly zero and -0 coordinates (zero rows / columns of A: zero numerators at the converted
                  quotients, zero quaternion components at the read-out);
      hostile     ordinary frames with a NaN / +-inf / 2^+-100 frame at lanes 0 and 63.

    What the library frames do NOT pin down: the small values of low_state are Gaussian noise scaled to 2^(edge - 1 ..
    edge + 1), so the lower edges are straddled statistically, not placed on an exact binade, and no frame aims a
    read-out's quaternion component at 2^-76 (only exact zeros and -0 reach that test through the library).  The exact
    edges -- inside, on and outside, for the pass, the reflector and the read-out -- are the tool's [G] [P] [T] [X]
    checks, which compare each site with its own a / b form on the device, not with the oracle.

Mutants run against this file on the device (profiles/r22/single_quotients/mutants.txt has the failing ids): the
correction dropped (21 of 24 tests fail); a window edge moved a binade outward, and a -0 numerator admitted (the tool
test fails: the edges are conservative, so the library tests cannot see them); the per-pass fallback redoing one
quotient instead of its group (the tool's [P] fails, on its all-denormal operand sets).
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import golden
import test_gpu_fit_division as fd

FAMILIES = ["low_state", "tiny", "mixed", "zeros", "hostile"]
NF = len(FAMILIES)
LATENCY_MAX_B = fd.LATENCY_MAX_B
N0 = 64 * 4 * NF + 513
BATCHES = (2, 65, LATENCY_MAX_B + 1, LATENCY_MAX_B + 65)
EDGES = (-46, -76)


def _family_of(i):
    return (i // 64) % NF if i < 64 * 4 * NF else i % NF


def _low_state(Z, i, rng):
    """A near-rank-1 (i even) or near-diagonal fit whose small values, noise 2^-j under a norm near 2^k, sit at
    2^(edge - 1 .. edge + 1)."""
    edge = EDGES[(i // 2) % 2] + (i // 4) % 3 - 1
    k = (-36, -20, 0)[(i // 12) % 3]
    j = k - edge
    n = len(Z)
    if i % 2:
        M = Z.astype(np.float64) * rng.uniform(0.5, 2.0, 3) * 8.0 + np.ldexp(rng.normal(size=(n, 3)), -j)
    else:
        M = rng.normal(size=(n, 1)) * rng.normal(size=3) * 4.0 + np.ldexp(rng.normal(size=(n, 3)), -j)
    return np.ldexp(M, k).astype(np.float32)


def _points(fam, Z, i, rng):
    if fam == "low_state":
        return _low_state(Z, i, rng)
    if fam == "tiny":
        M = fd._family_points("near_diag" if i % 2 else "near_rank1", Z, i // 2, rng)
        return np.ldexp(M, (-36, -30, 0, 30, 36)[(i // 132) % 5]).astype(np.float32)
    if fam == "mixed":
        return _low_state(Z, i // 2, rng) if i % 2 else fd._family_points("hostile", Z, i, rng)
    if fam == "zeros":
        return fd._family_points("zero_line", Z, i, rng)
    return fd._family_points("hostile", Z, i, rng)


@pytest.fixture(scope="module")
def kabsch_sets():
    import oracle as orc
    rng = np.random.default_rng(2222)
    out = {}
    for npts in (3, 5):
        n = 4096 + 65
        Z = (rng.standard_normal((n, npts, 3)) * 0.1).astype(np.float32)
        M = np.empty_like(Z)
        for i in range(n):
            fam = FAMILIES[_family_of(i)]
            if fam == "zeros" and (i // 12) % 2:
                Z[i, :, (i + 2) % 3] = [0.0, -0.0][(i // 24) % 2]
            M[i] = _points(fam, Z[i], i // NF if i >= 64 * 4 * NF else i, rng)
            if fam == "hostile":
                M[i] = fd._make_hostile(M[i], i, rng)
        out[npts] = (Z, M, orc.cal_joint_quat(Z, M))
    return out


@pytest.fixture(scope="module")
def fit_frames():
    """N0 golden frames with the three fits' points overwritten, repeated past the side kernel's smallest batch, and
    the oracle's result for both gripper modes (computed once on the N0: frames are independent)."""
    import oracle as orc
    zp = golden("zero_pose")
    zl = zp["vtrdyn_full_local_t"]
    g = golden("full_body_pos_precise")
    idx0 = np.arange(N0) % len(g["body"])
    body, lh, rh = (np.ascontiguousarray(g[k][idx0]) for k in ("body", "lh", "rh"))
    rng = np.random.default_rng(7722)
    Zt, Zl, Zr = zl[list(fd.TORSO_Z)], zl[list(fd.LEFT_Z)], zl[list(fd.RIGHT_Z)]
    for i in range(N0):
        fam = FAMILIES[_family_of(i)]
        which = (i // 64 // NF) % 3 if i < 64 * 4 * NF else (i // NF) % 3    # 0 torso, 1 wrists, 2 all three fits
        v = i // NF if i >= 64 * 4 * NF else i
        hostile = (lambda M: fd._make_hostile(M, i, rng)) if fam == "hostile" else (lambda M: M)
        if which in (0, 2):
            body[i, 10] = 0.0
            body[i, fd.TORSO_JOINTS, :] = hostile(_points(fam, Zt, v, rng))
        if which in (1, 2):
            for h, Zh in ((lh, Zl), (rh, Zr)):
                h[i, 0] = 0.0
                h[i, fd.WRIST_JOINTS, :] = hostile(_points(fam, Zh, v, rng))
    idx = np.arange(LATENCY_MAX_B + 65) % N0
    out = dict(ins=(body[idx], lh[idx], rh[idx]), n0=(body, lh, rh), ref={}, status={}, dof0={})
    for precise in (True, False):
        odof, olr, obr = orc.full_body_pos(zl, zp["vtrdyn_full_global_t"], body, lh, rh, precise)
        out["ref"][precise] = (odof[idx], olr[idx], obr[idx])
        out["status"][precise] = orc.frame_status(odof)[idx]
        out["dof0"][precise] = odof
    return out


def test_oracle_solves_or_raises_on_every_committed_frame(kabsch_sets, fit_frames):
    """On the CPU: a unit quaternion for every fit with finite points and NaN otherwise; the solver's oracle raises
    (status) on every NaN frame and on no finite one, with finite DOFs for every finite frame, in both gripper modes."""
    hostile = FAMILIES.index("hostile")
    for npts, (Z, M, q) in kabsch_sets.items():
        fam = np.array([_family_of(i) for i in range(len(M))])
        finite_in = np.isfinite(M).all(axis=(1, 2))
        assert finite_in[fam != hostile].all()
        ok = np.isfinite(q).all(axis=1)
        assert ok[finite_in & (fam != hostile)].all(), npts
        assert not ok[~finite_in].any(), npts
        assert np.abs(np.linalg.norm(q[ok].astype(np.float64), axis=1) - 1.0).max() < 1e-5, npts
    body, lh, rh = fit_frames["n0"]
    pts = np.concatenate([a.reshape(N0, -1) for a in (body, lh, rh)], axis=1)
    nan_in, finite_in = np.isnan(pts).any(axis=1), np.isfinite(pts).all(axis=1)
    assert nan_in.sum() >= 2 and (~finite_in & ~nan_in).sum() >= 2              # NaN and inf frames are there
    for precise in (True, False):
        st, odof = fit_frames["status"][precise][:N0], fit_frames["dof0"][precise]
        assert (st[nan_in] != 0).all() and (st[finite_in] == 0).all(), precise
        assert np.isfinite(odof[finite_in]).all(), precise


@pytest.mark.gpu
def test_check_fdiv1_single_on_the_device(gpu):
    import __graft_entry__ as ge
    csrc = os.path.join(ge.PKG, "csrc")
    deps = [ge.FDIV1_SRC] + [os.path.join(csrc, f) for f in ("rtg_math.cuh", "rtg_knobs.h", "rtg_crmath.h")]
    exe = ge.FDIV1_BIN
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        ge.build_fdiv1_check()
    r = subprocess.run([exe, "single"], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    assert "RTG_FDIV_CORRECTIONS = 1, RTG_FIT_FAST_DIV_TU = 1" in out, out
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("[")]
    assert len(lines) == 5 + 2 + 5 and all(" 0 mismatches" in ln and re.search(r"[ (]0 verdicts differ", ln) for ln in lines), out
    inreg = {ln.split("]")[0] + "]": int(re.search(r"in-region (\d+)", ln).group(1)) for ln in lines if "in-region" in ln}
    for f in range(3):   # five of the fifteen numerators are inside, for every mantissa of an in-region denominator
        assert inreg[f"[N.{f}]"] == 5 << 23, out
    assert inreg["[N.3]"] == 0 and inreg["[N.4]"] == 0, out          # a binade outside: the fallback ran for all
    for k in range(2):   # 2^-76 .. 2^94 inclusive, both signs; every other numerator took the fallback
        assert inreg[f"[C.{k}]"] == 2 * (((94 + 76) << 23) + 1), out
        assert re.search(rf"\[C\.{k}\].*: 4294967296 quotients, 0 mismatches", out), out
    for ln in lines[7:]:   # each site's test passed on some operand sets and refused others
        n, ok = int(re.search(r": (\d+) operand sets", ln).group(1)), int(re.search(r"test passed on (\d+)", ln).group(1))
        assert n == 1 << 24 and (1 << 20) <= ok <= n - (1 << 20), ln


@pytest.mark.gpu
@pytest.mark.parametrize("npts", [3, 5])
def test_cal_joint_quat_at_the_new_tests_vs_oracle(gpu, kabsch_sets, npts):
    from rtg import ops
    Z, M, o = kabsch_sets[npts]
    for n in (len(Z), 65, 1):
        g = ops.cal_joint_quat(Z[:n], M[:n]).cpu().numpy()
        bad = np.nonzero((fd._bits(g) != fd._bits(o[:n])).any(axis=1))[0]
        assert bad.size == 0, (npts, n, bad.size, bad[:8], [FAMILIES[_family_of(int(i))] for i in bad[:8]])


def _solver(precise):
    from rtg import _lib, assets
    from rtg.runtime import Solver
    zp = golden("zero_pose")
    return Solver(_lib.SOLVER_FULL_BODY_POS, zp["vtrdyn_full_local_t"], zp["vtrdyn_full_global_t"],
                  assets.parents("vtrdyn_full"), precise)


def _check(S, fr, precise, layout, sl, tag):
    from rtg.runtime import frame_status
    dev = [torch.from_numpy(np.ascontiguousarray(a[sl])).cuda() for a in fr["ins"]]
    if layout == "soa":
        dev = [t.permute(1, 2, 0).contiguous() for t in dev]
    dof, lr, br = S.retarget(dev, want_local_rot=True, want_body_rot=True, layout=layout)
    ref = fr["ref"][precise]
    np.testing.assert_array_equal(frame_status(dof).cpu().numpy(), fr["status"][precise][sl], err_msg=f"{tag}: status")
    for name, got, want in (("dof", dof, ref[0]), ("local_rot", lr, ref[1]), ("body_rot", br, ref[2])):
        bad = np.nonzero((fd._bits(got.cpu().numpy()) != fd._bits(want[sl])).reshape(len(want[sl]), -1).any(axis=1))[0]
        assert bad.size == 0, (tag, name, bad.size, bad[:8], [FAMILIES[_family_of(int(i) % N0)] for i in bad[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("precise", [True, False])
@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("B", BATCHES)
def test_fits_at_the_new_tests_vs_oracle(gpu, fit_frames, layout, B, precise):
    from rtg import _lib
    assert _lib.build_info()["knobs"]["RTG_LATENCY_MAX_B"] == LATENCY_MAX_B
    _check(_solver(precise), fit_frames, precise, layout, slice(0, B), f"B={B} {layout} precise={precise}")


@pytest.mark.gpu
@pytest.mark.parametrize("precise", [True, False])
@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_fits_at_the_new_tests_single_frame_vs_oracle(gpu, fit_frames, layout, precise):
    """B = 1 (k_fbp_frame1): a frame of every whole-wave (fit, family) pair, lanes 0 and 63 of the hostile waves, and
    a stretch of the mixed tail."""
    S = _solver(precise)
    frames = [64 * w + 5 for w in range(4 * NF)] + [64 * w + l for w in range(4 * NF) if w % NF == NF - 1 for l in (0, 63)]
    frames += list(range(64 * 4 * NF, 64 * 4 * NF + 2 * NF))
    for i in frames:
        _check(S, fit_frames, precise, layout, slice(i, i + 1), f"frame {i} {layout} precise={precise}")

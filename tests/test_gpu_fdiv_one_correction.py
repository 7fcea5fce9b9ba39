"""fdiv_n with ONE residual correction per quotient (csrc/rtg_math.cuh, RTG_FDIV_CORRECTIONS = 1) and the exp-map
read-out's unscaled square root cr_sqrt_nt(1 - w w), on the device against the compiler's IEEE a / b and
__builtin_sqrtf: the sampled form of tools/check_fdiv1.hip (built with the library's flags by
__graft_entry__.build_fdiv1_check).  The proof that one correction is enough is that tool's exhaustive run over all
2^46 mantissa pairs, whose log is profiles/r18/check_fdiv1.log; this test keeps the library's sequence on it:

  [1]    2^30 hashed in-window groups, fdiv_n<2> and fdiv_n<3>;
  [2.k]  every mantissa of the denominator (2^23 each) in [1, 2), in the window's lowest and highest binades, and
         in [1, 2) under one fixed numerator;
  [3.k]  round 13's nine families outside the window [2^-47, 2^47]: every group must take the a / b fallback;
  [R]    cr_sqrt_nt(1 - w w) == __builtin_sqrtf == cr_sqrt for every f32 w.

Zero mismatches required.  Mutant this fails on (profiles/r18/mutants.txt): both residual corrections dropped
(RTG_FDIV_CORRECTIONS = 0)."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_one_correction_fdiv_n_and_read_out_sqrt_equal_ieee_on_the_device(gpu):
    import __graft_entry__ as ge
    csrc = os.path.join(ge.PKG, "csrc")
    deps = [ge.FDIV1_SRC] + [os.path.join(csrc, f) for f in ("rtg_math.cuh", "rtg_knobs.h", "rtg_crmath.h")]
    exe = ge.FDIV1_BIN
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        ge.build_fdiv1_check()
    r = subprocess.run([exe, "sampled"], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    assert "RTG_FDIV_CORRECTIONS = 1, RTG_FIT_FAST_DIV_TU = 1" in out, out   # the library's own sequence was checked
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("[")]
    assert len(lines) == 1 + 4 + 9 + 1 and all(" 0 mismatches" in ln for ln in lines), out
    tag = lambda ln: ln.split("]")[0] + "]"
    fallback = {tag(ln): int(re.search(r"fallback on (\d+)", ln).group(1)) for ln in lines if "fallback on" in ln}
    groups = {tag(ln): int(re.search(r": (\d+) groups", ln).group(1)) for ln in lines if "fallback on" in ln}
    assert groups["[1]"] == 1 << 30 and fallback["[1]"] == 0, out
    for f in range(4):   # every mantissa, nothing inside the window takes the fallback
        assert groups[f"[2.{f}]"] == 1 << 23 and fallback[f"[2.{f}]"] == 0, out
    for f in range(9):   # outside it every group does
        assert fallback[f"[3.{f}]"] == groups[f"[3.{f}]"] > 0, out
    assert re.search(r"\[R\].*: 4294967296 inputs, 0 mismatches", out), out

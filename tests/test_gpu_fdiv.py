"""The shared-reciprocal division fdiv_n and the unscaled square root cr_sqrt_nt of csrc/rtg_math.cuh, checked on the
device against the compiler's IEEE division and __builtin_sqrtf by tools/check_fdiv.hip (built with the library's
flags by __graft_entry__.build_fdiv_check): 2^32 in-window groups, every mantissa of the denominator at the window's
edge binades, the families outside the window, special values, and every bit pattern cr_sqrt_nt may be given.

Mutants this fails on (profiles/r13/mutants.txt): guard always true, fallback removed, both residual corrections
dropped, the reciprocal's refinement dropped.  It does NOT fail with only the second residual correction dropped: on
every input above the quotient after one correction already equals the IEEE one, so no input here can tell."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_fdiv_n_and_cr_sqrt_nt_equal_ieee_on_the_device(gpu):
    import __graft_entry__ as ge
    csrc = os.path.join(ge.PKG, "csrc")
    deps = [ge.FDIV_SRC] + [os.path.join(csrc, f) for f in ("rtg_math.cuh", "rtg_knobs.h", "rtg_crmath.h")]
    exe = ge.FDIV_BIN
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        ge.build_fdiv_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("[")]
    assert len(lines) == 14 and all(" 0 mismatches" in ln for ln in lines), out
    tag = lambda ln: ln.split("]")[0] + "]"
    fallback = {tag(ln): int(re.search(r"fallback on (\d+)", ln).group(1)) for ln in lines if "fallback on" in ln}
    groups = {tag(ln): int(re.search(r": (\d+) (?:groups|triples)", ln).group(1)) for ln in lines if "fallback on" in ln}
    # inside the window nothing takes the fallback; outside it every group does
    assert fallback["[1]"] == 0 and fallback["[2]"] == 0, out
    for f in range(9):
        assert fallback[f"[3.{f}]"] == groups[f"[3.{f}]"] == 1 << 24, out
    assert 0 < fallback["[3.9]"] <= groups["[3.9]"] and 0 < fallback["[3b]"] < groups["[3b]"], out

"""Record what torch's MKL VML (VML_HA acos / sin / cos / sqrt) returns at every call the VML attribution tests make,
into tests/golden/vml_recorded.npz, so that those tests replay VML's values on any host.

VML's bits depend on the CPU MKL dispatches for: the goldens are the reference's run on an AVX-512 Intel host, and
only such a host reproduces them.  Run this there (python tools/record_vml.py).  It routes the live VML into the
oracle with every call logged (oracle_vml_log_all), runs

  A  every solver golden with VML at all sites   (test_vml_attribution) -- and refuses to write the file unless the
     goldens come out bit for bit, and
  B  each over-tolerance frame of profiles/r05/vml_attrib.json with VML logged but used nowhere
     (test_vml_attribution_one_call_per_frame: the inputs its single VML call sees),

and stores, per function, the distinct inputs at which VML's result is not the correctly rounded one (input bits
ascending, with VML's output bits): <fn>_x, <fn>_y (uint32).  Everywhere else VML returned what the oracle computes
itself, (float)f((double)x).
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import test_oracle_golden as T  # noqa: E402  (its conftest sets the import paths)

import oracle as orc  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "vml_recorded.npz")
REC = np.dtype([("site", "<i4"), ("call", "<i4"), ("x", "<u4"), ("cr", "<u4"), ("vml", "<u4")])
SITE_FN = ["sin", "cos", "sqrt", "sqrt", "acos", "sin", "cos", "acos"]   # rtg_oracle.c VS_*: the function of each site
CAP = 4_000_000


def main():
    fns = T._torch_vml()
    cpu = open("/proc/cpuinfo").read()
    if fns is None or "avx512f" not in cpu or "GenuineIntel" not in cpu:
        sys.exit("needs torch's MKL VML on an AVX-512 Intel host (the goldens' ISA)")
    lib = orc.lib()
    buf = np.zeros(CAP, REC)
    recs = []

    def logged(fn):
        lib.oracle_vml_log(buf.ctypes.data_as(ctypes.c_void_p), CAP)
        out = fn()
        n = lib.oracle_vml_log_count()
        assert n < CAP, "log full"
        recs.append(buf[:n].copy())
        return out

    lib.oracle_set_threads(1)
    lib.oracle_set_vml(*fns[:3], ctypes.c_longlong(0x140102))   # VML_HA | VML_FTZDAZ_OFF | VML_ERRMODE_IGNORE
    lib.oracle_set_vml_sqrt(fns[3])
    lib.oracle_vml_log_all(1)
    try:
        for name in T.BOUNDS:                                    # A
            dof, d = logged(lambda: T._run(name))
            np.testing.assert_array_equal(dof, d["dof"], err_msg=f"{name}: this host's VML is not the goldens'")
        lib.oracle_set_vml_sites(ctypes.c_uint32(0))             # B
        rep = json.load(open(os.path.join(REPO, "profiles", "r05", "vml_attrib.json")))
        for name, sol in rep["solvers"].items():
            for fr in sol["over_tol"]:
                logged(lambda: T._solve_frames(name, np.array([fr["frame"]])))
    finally:
        lib.oracle_vml_log(None, 0)
        lib.oracle_vml_log_all(0)
        lib.oracle_set_vml_sites(ctypes.c_uint32(0xFFFFFFFF))
        lib.oracle_set_vml(None, None, None, ctypes.c_longlong(0))
        lib.oracle_set_vml_sqrt(None)
        lib.oracle_set_threads(os.cpu_count() or 1)
    r = np.concatenate(recs)
    assert (r["site"] < len(SITE_FN)).all(), "a call outside the solver path's sites"
    fn_of = np.array(SITE_FN)[r["site"]]
    out = {}
    for fn in ("acos", "sin", "cos", "sqrt"):
        m = (fn_of == fn) & (r["vml"] != r["cr"])
        x, i = np.unique(r["x"][m], return_index=True)
        y = r["vml"][m][i]
        assert all((r["vml"][m][r["x"][m] == v] == w).all() for v, w in zip(x, y))   # a function of x
        out[f"{fn}_x"], out[f"{fn}_y"] = x, y
        print(f"{fn}: {int((fn_of == fn).sum())} calls, VML not correctly rounded at {int(m.sum())} of them, "
              f"{len(x)} distinct inputs")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

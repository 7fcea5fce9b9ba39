"""The handle constructors' failure path under ASan / UBSan, as a stand-alone program (tests/api_lifetime_check.cpp
with its own main, csrc/rtg_api.cpp compiled with the host sanitizers, the kernel objects as built): on a machine
without a device every constructor fails at its first device call, and whatever it had acquired by then has to be
released by the owners alone.  Nothing is loaded into this process and nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

import build_recipe
from conftest import PKG, REPO

CSRC = os.path.join(PKG, "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# each constructor's first device call (the label of hip_check's message)
FIRST_LABEL = {"rtg_topology_create": "hipMalloc(parents)", "rtg_motion_lib_create": "hipMalloc(motion clip table)",
               "rtg_rot_ingest_create": "hipMalloc(rot ingest blob)", "rtg_solver_create": "hipMalloc(solver consts)",
               "rtg_server_inbox_alloc": "hipExtMallocWithFlags(inbox)"}
DEVICE = 2   # RTG_ERR_DEVICE


def kernel_objects():
    """The kernel objects as built: the Makefile's list (tests/test_build_recipe_host.py holds it to the record)."""
    return [os.path.join(CSRC, t + ".o") for t in build_recipe.kernel_tus()]


def test_constructors_fail_clean_without_a_device(tmp_path):
    """Exit status 0, nothing from the sanitizers, every constructor RTG_ERR_DEVICE with its first label (each one
    twice), *out NULL after each failure (the program checks that), every destructor fine with NULL."""
    from rtg import _lib
    if _lib.lib().rtg_device_count() != 0:
        pytest.skip("a device is visible: the no-device failure path cannot be reached (and a sanitizer build never "
                    "runs with a GPU open)")
    objs = kernel_objects()
    if not all(os.path.exists(o) for o in objs):
        pytest.skip("the kernel objects are not built (make -C humanoid-real-time-retarget_amd/csrc)")
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    clangxx = shutil.which("clang++") or os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin",
                                                      "clang++")
    inc = os.path.join(REPO, "include")
    api_o, main_o, exe = (str(tmp_path / n) for n in ("rtg_api_san.o", "main.o", "check"))
    # the Makefile's line for rtg_api.o at -O1 -g, the sanitizers on the host side only
    src, flags = build_recipe.recipe()["rtg_api.o"]
    assert "-O3" in flags
    subprocess.run([hipcc, *("-O1" if f == "-O3" else f for f in flags), "-g", "-Xarch_host", SAN[0], "-Xarch_host",
                    SAN[1], src, "-o", api_o], check=True, timeout=300, cwd=CSRC)
    subprocess.run([clangxx, "-g", "-O1", *SAN, "-I", inc, "-c", os.path.join(REPO, "tests", "api_lifetime_check.cpp"),
                    "-o", main_o], check=True, timeout=120)
    # objects only on this line: after a .cpp hipcc would read them as HIP source
    subprocess.run([hipcc, "--offload-arch=gfx950", SAN[0], main_o, api_o, *objs, "-o", exe], check=True, timeout=300)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr.strip() == "", r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    seen = {}
    for ln in lines[:-1]:
        name, rc, msg = ln.split(" ", 2)
        seen.setdefault(name, []).append((int(rc), msg))
    for name, label in FIRST_LABEL.items():
        want = 8 if name == "rtg_solver_create" else 2   # every constructor twice; four solver kinds
        assert len(seen[name]) == want, (name, seen[name])
        for rc, msg in seen[name]:
            assert rc == DEVICE and msg.startswith(label + ": "), (name, rc, msg)
    for name in ("rtg_dof_model_create(NULL)", "rtg_retarget_plan_create(NULL)"):
        assert [rc for rc, _ in seen[name]] == [1, 1] and all("NULL topology" in m for _, m in seen[name]), seen[name]
    for name in ("rtg_topology_destroy(NULL)", "rtg_dof_model_destroy(NULL)", "rtg_retarget_plan_destroy(NULL)",
                 "rtg_solver_destroy(NULL)", "rtg_server_inbox_free(NULL)"):
        assert seen[name] == [(0, "")], (name, seen[name])
    assert lines[-1] == "void destructors took NULL"

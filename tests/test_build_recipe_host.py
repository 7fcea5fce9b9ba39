"""csrc/Makefile is the one recipe for the library, its variants and the tests' own builds: the flags of every object
are held to tests/golden/build_recipe.json, recorded (tools/record_build_recipe.py) from the Makefile that still wrote
each rule out by hand.  The bits and the speed of a kernel depend on these flags as much as on its source (DESIGN.md
5), so a flag that changes here changes on purpose, with the record.  Nothing is compiled: make only prints."""
import json
import os
import subprocess

import build_recipe as br

with open(br.GOLDEN) as _f:
    RECORD = json.load(_f)["objects"]
PRODUCT = {o: f for o, f in RECORD.items() if os.path.dirname(o) == ""}


def test_makefile_compiles_every_object_as_recorded():
    """The reporting target names the same objects (the twelve of the product, the recompiled ones of `make
    variants`) and gives each the same flags."""
    got = br.recorded_form(br.recipe())
    assert sorted(got) == sorted(RECORD)
    for obj in RECORD:
        assert got[obj] == RECORD[obj], obj


def test_variant_script_builds_the_product_plus_its_defines():
    """tools/build_variants.sh, with make told to print only (MAKEFLAGS=n): every object of the product, each with
    the product's flags for that unit plus the spec's defines, and one link of them all."""
    defs = ["-DRTG_EXP_NO_TABLE=1", "-DRTG_PROBE=2"]
    env = dict(os.environ, MAKEFLAGS="n", HIPCC=br.HIPCC)
    for k in ("NOSLP_TUS", "IEEE_DIV_TUS", "JOBS"):
        env.pop(k, None)
    r = subprocess.run([os.path.join(br.REPO, "tools", "build_variants.sh"), "probe:" + " ".join(defs)], check=True,
                       text=True, capture_output=True, timeout=60, env=env)
    got = br.recorded_form(br.compile_lines(r.stdout.splitlines()))
    want = {os.path.join("..", "variants", "obj_probe", o): sorted(f + defs) for o, f in PRODUCT.items()}
    assert sorted(got) == sorted(want)
    for obj in want:
        assert got[obj] == want[obj], obj
    link = [ln.split() for ln in r.stdout.splitlines() if " -shared " in ln]
    assert len(link) == 1 and link[0][-2:] == ["-o", "../variants/probe.so"], link
    assert sorted(t for t in link[0] if t.endswith(".o")) == sorted(want)
    assert not os.path.exists(os.path.join(br.CSRC, "..", "variants", "obj_probe")), "printing only"


def test_lifetime_check_links_the_makefiles_kernel_objects():
    """tests/test_api_lifetime_host.py links the kernel objects as built: its list is the product's objects without
    the C ABI's, which it compiles itself from the Makefile's line."""
    from test_api_lifetime_host import kernel_objects
    objs = kernel_objects()
    assert all(os.path.dirname(o) == br.CSRC for o in objs)
    assert sorted([os.path.basename(o) for o in objs] + ["rtg_api.o"]) == sorted(PRODUCT)

#!/usr/bin/env python3
"""Record how csrc/Makefile compiles each object of librtg_hip.so and of the `make variants` libraries into
tests/golden/build_recipe.json: per object its flags as a sorted list (tests/build_recipe.py says what is left out).
tests/test_build_recipe_host.py holds the Makefile, tools/build_variants.sh and the tests' own builds to this record,
so run this only when a flag is meant to change, and say in the commit which one and what it measured.
The record was first taken from the compile lines of `make -n -B all variants` with the Makefile that wrote each rule
out by hand (profiles/r19/recipe/NOTES.md)."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import build_recipe as br   # noqa: E402

if __name__ == "__main__":
    objects = br.recipe()
    with open(br.GOLDEN, "w") as f:
        json.dump({"objects": br.recorded_form(objects)}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(objects)} objects -> {os.path.relpath(br.GOLDEN)}")

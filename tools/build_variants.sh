#!/usr/bin/env bash
# Build librtg variants with measurement knobs into humanoid-real-time-retarget_amd/variants/<name>.so
# usage: tools/build_variants.sh "name:-DKNOB=1 -DOTHER=0" ...   (time them with tools/variant_bench.sh)
# The knobs are those of csrc/rtg_knobs.h.  A variant that was measured and rejected has no knob any more: its branch
# was removed from the source (DESIGN.md keeps the numbers, git history the code), so build it from that commit.
# A variant is the product plus its defines: csrc/Makefile compiles every unit with the product's own flags and the
# spec's -D... into variants/obj_<name>/.  NOSLP_TUS / IEEE_DIV_TUS (environment) override the Makefile's lists.
# A variant built with a wrong-answer knob (RTG_EXP_STUB_SVD / _NO_TABLE / _HOT_INPUTS) reports it in
# rtg_build_info(); rtg._lib refuses to load it unless RTG_ALLOW_MEASUREMENT_BUILD=1 (variant_bench.sh sets it).
set -eu
csrc="$(dirname "$0")/../humanoid-real-time-retarget_amd/csrc"
for spec in "$@"; do
  name="${spec%%:*}"; defs="${spec#*:}"
  make -C "$csrc" -j"${JOBS:-8}" all OBJDIR="../variants/obj_$name" OUT="../variants/$name.so" DEFS="$defs" \
    ${NOSLP_TUS+NOSLP_TUS="$NOSLP_TUS"} ${IEEE_DIV_TUS+IEEE_DIV_TUS="$IEEE_DIV_TUS"}
  echo "built variants/$name.so ($defs)"
done

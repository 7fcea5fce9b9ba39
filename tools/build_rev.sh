#!/usr/bin/env bash
# Build librtg_hip.so from the csrc/ + include/ of a git revision into humanoid-real-time-retarget_amd/variants/<name>.so
# (the A/B base for tools/ab_headline.py: same box, same session, interleaved).  Build container only.
# The revision's own Makefile builds it, so the base is that revision as it ships: its units, its per-unit flags.
# usage: tools/build_rev.sh <rev> <name> [extra hipcc flags]
set -eu
rev=$1; name=$2; shift 2
repo="$(cd "$(dirname "$0")/.." && pwd)"
out="$repo/humanoid-real-time-retarget_amd/variants/$name.so"
tmp=$(mktemp -d)
git -C "$repo" archive "$rev" humanoid-real-time-retarget_amd/csrc include | tar -x -C "$tmp"
cd "$tmp/humanoid-real-time-retarget_amd/csrc"
mkdir -p "$(dirname "$out")"
rm -f "$out"
make -j"${JOBS:-8}" all OUT="$out" HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}${*:+ $*}"
[ -f "$out" ] || cp ../librtg_hip.so "$out"   # a revision whose Makefile has a fixed OUT
rm -rf "$tmp"
echo "built variants/$name.so from $rev"

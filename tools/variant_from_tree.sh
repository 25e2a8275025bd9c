#!/bin/bash
# Build a measurement library from another copy of the sources (e.g. a git revision), for A/B runs
# against the working tree with tools/ab.py (never shipped):
#   tools/variant_from_tree.sh NAME REV [FLAGS]   -> tools/variants/libfcs_NAME.so built from `git show REV:...`
# The revision's own nstack_amd/Makefile builds it: its SRC list and its flags. FLAGS ride on the
# compiler command, so they reach the link line as well as every compile (harmless for -D switches).
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(dirname "$HERE")
name=$1; rev=$2; flags=${3:-}
tmp=$(mktemp -d)
mkdir -p "$tmp/nstack_amd/csrc" "$tmp/include" "$HERE/variants"
for f in nstack_amd/Makefile $(git -C "$ROOT" ls-tree --name-only "$rev" nstack_amd/csrc/ include/); do
  git -C "$ROOT" show "$rev:$f" > "$tmp/$f"
done
make -s -j8 -C "$tmp/nstack_amd" HIPCC="/opt/rocm/bin/hipcc $flags" "$tmp/nstack_amd/libnstack_fcs.so"
cp "$tmp/nstack_amd/libnstack_fcs.so" "$HERE/variants/libfcs_$name.so"
rm -rf "$tmp"
ls -la "$HERE/variants/libfcs_$name.so"

#!/bin/bash
# Build the committed HEAD (or REV) library as abtest/base/libshdtopo.so: the "base" side of a
# same-box A/B against the working tree (tools/ab_probe.sh, tools/ab_replay.sh).  REV's own
# Makefile names its sources.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
REV=${1:-HEAD}
TMP=$(mktemp -d)
git -C "$ROOT" archive "$REV" shadow_amd/csrc include | tar -x -C "$TMP"
OUT=$ROOT/abtest/base
mkdir -p "$OUT"
make -s -j"$(nproc | awk '{print ($1 < 16) ? $1 : 16}')" -C "$TMP/shadow_amd/csrc" \
  OBJDIR="$TMP/obj" OUT="$OUT" "$OUT/libshdtopo.so"
rm -rf "$TMP"
echo "$OUT/libshdtopo.so ($REV)"
